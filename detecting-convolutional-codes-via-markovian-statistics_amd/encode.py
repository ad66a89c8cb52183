"""Convolutional encoder on the device: the inverse of the decoders in decode.py.

cvd_encode_frames (include/cvd.h; HIP kernels in csrc/cvd_encode.hip) turns F rows of packed
information bits -- the `bits` of every frames decoder, or rows made by pack_info -- into one
capture in any format the decoders read: open, terminated or tail-biting frames, punctured or
not, at a stride or at offsets.  So decode(encode(u)) == u and encode(decode(y)) ^ y (where the
channel errors are) are one call each.  encode_frames is the batch call, encode_capture the
single open stream.  Exact; no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .codes import as_code
from .decode import MAX_T, puncture_pattern, punctured_bits
from .detector import _require_gpu, _stream_ptr

ENCODE_MODES = {"open": 0, "terminated": 1, "tail-biting": 2, "tailbiting": 2}   # CVD_ENCODE_*
CAPTURE_SOFT = 3                                                                 # CVD_CAPTURE_SOFT
ENCODE_FORMATS = dict(_lib.CAPTURE_FORMATS, soft=CAPTURE_SOFT)
MAX_M = 16


def pack_info(u):
    """0/1 array [F, T] or [T] -> rows of information bits as the library reads them: uint8
    [F, 4*ceil(T/32)] (or [4*ceil(T/32)]), bit t of a row = bit (t & 7) of byte t >> 3."""
    u = np.asarray(u)
    if u.ndim not in (1, 2) or ((u != 0) & (u != 1)).any():
        raise ValueError("pack_info takes a 0/1 array [F, T] or [T]")
    T = u.shape[-1]
    rows = np.zeros(u.shape[:-1] + ((T + 31) // 32 * 4,), np.uint8)
    p = np.packbits(u.astype(np.uint8), axis=-1, bitorder="little")
    rows[..., :p.shape[-1]] = p
    return rows


def unpack_info(rows, T):
    """The first T bits of each row of pack_info's layout (numpy or torch uint8), as a 0/1 array."""
    if isinstance(rows, torch.Tensor):
        rows = rows.cpu().numpy()
    rows = np.asarray(rows, np.uint8)
    return np.unpackbits(rows, axis=-1, bitorder="little")[..., :int(T)]


def _info_rows(info, T, F, dev):
    """(device uint8 tensor, its row pitch in words, F) of the information rows: a 2-D tensor on
    `dev` whose rows are contiguous, 4-byte aligned and a multiple of 4 bytes apart is used in
    place (a column of a list result), anything else is copied."""
    if isinstance(info, np.ndarray):
        info = torch.from_numpy(np.ascontiguousarray(info))
    if not isinstance(info, torch.Tensor) or info.dtype != torch.uint8:
        raise TypeError("info is a numpy array or torch tensor of uint8")
    if info.dim() == 1:
        info = info.reshape(1, -1)
    if info.dim() != 2 or info.shape[1] % 4:
        raise ValueError("info is [F, 4*pitch] bytes: rows of whole 32-bit words")
    w = (T + 31) // 32
    if info.shape[1] < 4 * w:
        raise ValueError(f"info rows of {info.shape[1]} bytes hold fewer than T = {T} bits")
    if F is None:
        F = info.shape[0]
    F = int(F)
    if not 0 <= F <= info.shape[0]:
        raise ValueError(f"F = {F} but info has {info.shape[0]} rows")
    info = info[:F]
    inplace = (info.device == dev and F > 0 and info.stride(1) == 1 and info.data_ptr() % 4 == 0
               and (F == 1 or (info.stride(0) % 4 == 0 and info.stride(0) >= 4 * w)))
    if not inplace:
        info = info.to(dev).contiguous()
    pitch = info.stride(0) // 4 if F > 1 else info.shape[1] // 4
    return info, pitch, F


def encode_frames(n, m, gen, info, T, F=None, mode="terminated", start_state=0, keep=None, format="bytes",
                  amplitude=None, start=0, stride=None, offsets=None, size=None, device=None):
    """cvd_encode_frames: F frames of T steps of the k = 1 code gen[j][i][d] (n in 2..3, m <= 16)
    from the rows of `info` (uint8 [F, 4*pitch], bit t of a row LSB first: a decoder's `bits`, a
    view res["bits"][:, i] of a list result, or pack_info's rows; bits at or past T are ignored).
    mode: "open" (the encoder starts in start_state), "terminated" (as open, and the last m inputs
    are taken as 0 whatever the row holds) or "tail-biting" (the encoder starts in the state it
    ends in).  keep: anything puncture_pattern takes; the pattern restarts in every frame.
    format: "bytes", "lsb", "msb" or "soft" (int8 +-amplitude, default 24; 0 where no frame lies).
    Frame f begins at position start + f*stride (stride=None: the span of a frame) or at
    offsets[f] (int64; bytes and soft only; a frame that does not lie inside the capture is
    skipped).  size: positions of the capture (None: the smallest that holds the frames).
    Returns a dict: capture (device uint8 / int8 tensor, every position no frame covers 0: ready
    for every decode_*), nbits (soft: nvals), format, span, stride, F, T, written, skipped."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    if mode not in ENCODE_MODES:
        raise ValueError(f"mode {mode!r}: one of open, terminated, tail-biting")
    if format not in ENCODE_FORMATS:
        raise ValueError(f"format {format!r}: one of {', '.join(ENCODE_FORMATS)}")
    fmt = ENCODE_FORMATS[format]
    if fmt == CAPTURE_SOFT:
        amplitude = 24 if amplitude is None else int(amplitude)
        if not 1 <= amplitude <= 127:
            raise ValueError(f"amplitude = {amplitude}: must be 1..127")
    elif amplitude is not None:
        raise ValueError("amplitude needs format=\"soft\"")
    code = as_code(gen, m, 1, n)
    if not 1 <= T <= MAX_T:
        raise ValueError(f"T = {T}: a frame has 1..2^31 - 1 steps")
    if keep is not None:
        keep = puncture_pattern(keep, n)
    span = n * T if keep is None else punctured_bits(T, keep)
    rows, pitch, F = _info_rows(info, T, F, dev)
    off = None
    if offsets is not None:
        off = torch.from_numpy(np.ascontiguousarray(offsets)) if isinstance(offsets, np.ndarray) else offsets
        if not isinstance(off, torch.Tensor) or off.dtype != torch.int64:
            raise TypeError("offsets is a numpy array or torch tensor of int64")
        off = off.reshape(-1).to(dev).contiguous()
        if off.numel() != F:
            raise ValueError(f"F = {F} but {off.numel()} offsets")
        start, stride = 0, span
        if size is None:
            size = int(off.max().item()) + span if F else 0
    else:
        start = int(start)
        stride = span if stride is None else int(stride)
        if size is None:
            size = start + (F - 1) * stride + span if F else 0
    size = max(int(size), 0)
    nbytes = size if fmt in (_lib.CAPTURE_BYTES, CAPTURE_SOFT) else (size + 7) // 8
    L = _lib.lib()
    with torch.cuda.device(dev):
        # F == 0: the call writes nothing, the capture is all zeros
        alloc = torch.zeros if F == 0 else torch.empty
        buf = alloc((nbytes + 15) // 16 * 16 or 16, dtype=torch.int8 if fmt == CAPTURE_SOFT else torch.uint8, device=dev)
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        _lib.check(L.cvd_encode_frames(code.c, bytes(keep) if keep is not None else None, len(keep) if keep is not None else 0,
                                       ctypes.c_void_p(rows.data_ptr()), pitch, F, T, ENCODE_MODES[mode], int(start_state),
                                       fmt, amplitude or 0, ctypes.c_void_p(buf.data_ptr()), size, start, stride,
                                       ctypes.c_void_p(off.data_ptr()) if off is not None else None,
                                       ctypes.c_void_p(stats.data_ptr()), _stream_ptr()))
        s = stats.cpu().tolist()     # synchronises: rows and off may be freed on return
    return {"capture": buf[:nbytes], "nbits": size, "format": format, "span": span, "stride": stride, "F": F, "T": T,
            "written": int(s[0]), "skipped": int(s[1])}


def encode_capture(n, m, gen, info, T=None, start_state=0, keep=None, format="bytes", amplitude=None, device=None):
    """One open stream (encode_frames with F = 1, mode "open"): `info` is LSB-packed bits as
    decode_capture's `bits` (any number of bytes; T=None: all of them), step t's coded bits at
    position n*t + j.  Returns encode_frames' dict with end_state, the last m inputs (bit 0 the
    most recent: the start_state that continues the stream)."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    if isinstance(info, np.ndarray):
        info = torch.from_numpy(np.ascontiguousarray(info))
    if not isinstance(info, torch.Tensor) or info.dtype != torch.uint8:
        raise TypeError("info is a numpy array or torch tensor of uint8")
    info = info.reshape(-1)
    T = 8 * info.numel() if T is None else int(T)
    if not 1 <= T <= 8 * info.numel():
        raise ValueError(f"T = {T} outside the {8 * info.numel()} bits of info")
    if info.numel() % 4:
        padded = torch.zeros((info.numel() + 3) // 4 * 4, dtype=torch.uint8, device=info.device)
        padded[:info.numel()] = info
        info = padded
    m = int(m)
    res = encode_frames(n, m, gen, info.reshape(1, -1), T, 1, "open", start_state, keep, format, amplitude, device=dev)
    lo = max(T - m, 0)
    tail = unpack_info(info[lo // 8:(T + 7) // 8], T - lo // 8 * 8)[lo % 8:]       # u_lo .. u_{T-1}
    state = int(start_state)
    for b in tail:
        state = ((state << 1) | int(b)) & ((1 << m) - 1)
    res["end_state"] = state
    return res

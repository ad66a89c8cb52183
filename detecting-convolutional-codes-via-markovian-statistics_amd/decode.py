"""Hard-decision Viterbi decoder of a captured bitstream (nothing in the reference, whose
Eq. 4-5 recursion keeps no survivor decisions): what was sent, and how noisy is the channel?

cvd_viterbi_decode (include/cvd.h; HIP kernels in csrc/cvd_decode.hip) runs the detector's
relative-metric recursion over the capture in parallel blocks, keeps the decisions and traces
the maximum-likelihood path back: the information bits, the Hamming distance of the path to
the capture (errors / (n T) is the estimate of the crossover probability that `scan` needs)
and its end states.  Exact: the result is the sequential decoder's whatever the block split;
the counters say how often the speculative blocks had to be redone.  No CPU fallback.

The workflow on a capture: identify (which code, which phase) -> decode (the data, p) ->
scan --p p.  The decoded bits are a format="lsb" capture themselves and can go straight back
into parity_sweep / find_parity_checks, e.g. when an outer code is present.
"""
import ctypes

import torch

from . import _lib
from .codes import as_code
from .detector import _require_gpu, _stream_ptr, capture_buffer

MAX_T = (1 << 31) - 1    # steps per cvd_viterbi_decode call (include/cvd.h)
# include/cvd.h CVD_VITERBI_BLOCK, CVD_VITERBI_WARM(m), CVD_VITERBI_DEPTH(m)
DEFAULT_BLOCK = 4096


def default_warm(m):
    return 64 * int(m)


def default_depth(m):
    return 24 * (int(m) + 2)


def decode_capture(n, m, gen, capture, start=0, T=None, format="bytes", nbits=None, block=None, warm=None,
                   depth=None, device=None):
    """cvd_viterbi_decode over a capture (numpy array or torch tensor of uint8, as
    Detector.pack_capture takes it) of the k = 1 code gen[j][i][d]: capture bit
    start + n*t + j is output j of step t.  T=None: as many whole symbols as fit from `start`.
    block / warm / depth None: the library's defaults.  Returns a dict: bits (device uint8
    tensor of ceil(T/32)*4 bytes, LSB-packed: with nbits=T a format="lsb" capture), T, errors,
    ber = errors / (n T) (0.0 at T = 0), start_state, end_state, blocks, forward_reruns,
    trace_fixups (how many blocks the forward pass / the traceback had to redo), block, warm,
    depth (as resolved)."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, start = int(n), int(m), int(start)
    code = as_code(gen, m, 1, n)
    cap, fmt, nbits = capture_buffer(capture, format, nbits, dev)
    if T is None:
        T = max(0, nbits - start) // n if start >= 0 else 0
    T = int(T)
    if T < 0:
        raise ValueError("T must be >= 0")
    if T > MAX_T:
        raise ValueError(f"T = {T}: one call decodes at most 2^31 - 1 steps")
    blk = 0 if block is None else int(block)
    wrm = -1 if warm is None else int(warm)
    dep = -1 if depth is None else int(depth)
    if (block is not None and blk <= 0) or (warm is not None and wrm < 0) or (depth is not None and dep < 0):
        raise ValueError("needs block > 0 (a multiple of 32), warm >= 0 and depth >= 0")
    L = _lib.lib()
    wbytes = int(L.cvd_viterbi_workspace_bytes(n, m, T, blk))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(L.cvd_viterbi_decode(code.c, None, 0, fmt, 0, 0, blk, wrm, dep, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        bits = torch.zeros((T + 31) // 32 * 4, dtype=torch.uint8, device=dev)
        stats = torch.zeros(9, dtype=torch.int64, device=dev)
        if T == 0:
            # no launch: validate the arguments, report the resolved defaults
            _lib.check(L.cvd_viterbi_decode(code.c, ctypes.c_void_p(cap.data_ptr()), nbits, fmt, start, 0, blk, wrm,
                                            dep, None, None, None, _stream_ptr()))
            s = [0, 0, 0, 0, 0, 0, blk or DEFAULT_BLOCK, default_warm(m) if wrm < 0 else wrm,
                 default_depth(m) if dep < 0 else dep]
        else:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"decode_capture: the workspace of T = {T} steps (m = {m}) is {wbytes} bytes, "
                                  f"{free} bytes of device memory are free: decode the capture in pieces")
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            _lib.check(L.cvd_viterbi_decode(code.c, ctypes.c_void_p(cap.data_ptr()), nbits, fmt, start, T, blk, wrm,
                                            dep, ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                                            ctypes.c_void_p(work.data_ptr()), _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap and work may be freed on return
    return {"bits": bits, "T": T, "errors": int(s[0]), "ber": s[0] / (n * T) if T else 0.0,
            "start_state": int(s[4]), "end_state": int(s[5]), "blocks": int(s[1]), "forward_reruns": int(s[2]),
            "trace_fixups": int(s[3]), "block": int(s[6]), "warm": int(s[7]), "depth": int(s[8])}

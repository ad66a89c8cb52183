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

Punctured captures (DVB-S, 802.11a: a periodic pattern leaves output bits out) go through
cvd_viterbi_decode_punctured (csrc/cvd_decode_punct.hip): puncture_pattern names the pattern,
decode_capture_punctured decodes, sync_punctured finds where the periods begin.

Soft captures (one int8 confidence value per channel bit, 0 = erased) go through
cvd_viterbi_decode_soft (csrc/cvd_decode_soft.hip): decode_capture_soft decodes, with keep=...
after depuncturing on the device (depuncture_soft); soft_from_bits turns hard bits into such a
capture and sync_punctured_soft is sync_punctured's loop.

Framed captures (802.11a/g PPDUs, GSM bursts, packets: each frame starts in a known state and
is driven back to one by m tail bits) go through cvd_viterbi_decode_frames and its punctured
and soft siblings (csrc/cvd_decode_frames.hip): decode_frames and decode_frames_soft decode a
batch of F frames of T steps, at a stride or at given offsets, in one call, with the start and
end states told to the decoder.

Punctured soft frames (what a receiver produces at the punctured rates) go through
cvd_viterbi_decode_frames_soft_punctured, _tailbiting_soft_punctured and _llr_punctured
(csrc/cvd_decode_psoft.hip): decode_frames_soft_punctured, decode_frames_tailbiting_soft_punctured
and decode_frames_llr_punctured.  The command line reaches the first (decode --frame T --format
soft --puncture SPEC); the tail-biting and soft-output ones are Python and C only.

List decoding (cvd_viterbi_decode_frames_list, csrc/cvd_decode_list.hip): decode_frames_list returns
the L best paths of every soft frame, frames_crc (cvd_frames_crc) checks rows of decoded bits against
a CRC on the device, and decode_frames_crc picks of every frame the first path that passes.
"""
import ctypes

import numpy as np
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


def _steps(T, block, warm, depth):
    """T, block, warm and depth as the library takes them: 0 / -1 ask for its defaults."""
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
    return T, blk, wrm, dep


def _decode(who, entry, workspace, lead, fmt, cap, nbits, start, n, m, T, blk, wrm, dep, nstats, warm0, depth0, dev,
            prepare=None):
    """One call of the library's decoder `entry`(*lead, capture, nbits, *fmt, start, T, block, warm,
    depth, bits, stats, work, stream) over T steps: (bits, the nstats stats as a list).  T == 0
    launches nothing: the call validates, and the stats report block, warm and depth as resolved
    (warm0 / depth0: the defaults).  prepare(lib) -> (cap, nbits, start), if given, runs behind
    the shape check.  `workspace` is the entry point that sizes d_work, `who` names the caller
    in the MemoryError."""
    L = _lib.lib()
    call = getattr(L, entry)
    wbytes = int(getattr(L, workspace)(n, m, T, blk))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(call(*lead, None, 0, *fmt, 0, 0, blk, wrm, dep, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        bits = torch.zeros((T + 31) // 32 * 4, dtype=torch.uint8, device=dev)
        stats = torch.zeros(nstats, dtype=torch.int64, device=dev)
        if prepare is not None:
            cap, nbits, start = prepare(L)
        if T == 0:
            # no launch: validate the arguments, report the resolved defaults
            _lib.check(call(*lead, ctypes.c_void_p(cap.data_ptr()), nbits, *fmt, start, 0, blk, wrm, dep, None, None,
                            None, _stream_ptr()))
            s = [0, 0, 0, 0, 0, 0, blk or DEFAULT_BLOCK, warm0 if wrm < 0 else wrm, depth0 if dep < 0 else dep]
            s += [0] * (nstats - len(s))
        else:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"{who}: the workspace of T = {T} steps (m = {m}) is {wbytes} bytes, "
                                  f"{free} bytes of device memory are free: decode the capture in pieces")
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            _lib.check(call(*lead, ctypes.c_void_p(cap.data_ptr()), nbits, *fmt, start, T, blk, wrm, dep,
                            ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                            ctypes.c_void_p(work.data_ptr()), _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap and work may be freed on return
    return bits, s


def _result(bits, T, s, errors, ber):
    """decode_capture's dict from the stats."""
    return {"bits": bits, "T": T, "errors": int(errors), "ber": ber,
            "start_state": int(s[4]), "end_state": int(s[5]), "blocks": int(s[1]), "forward_reruns": int(s[2]),
            "trace_fixups": int(s[3]), "block": int(s[6]), "warm": int(s[7]), "depth": int(s[8])}


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
    T, blk, wrm, dep = _steps(T, block, warm, depth)
    bits, s = _decode("decode_capture", "cvd_viterbi_decode", "cvd_viterbi_workspace_bytes", (code.c,), (fmt,), cap,
                      nbits, start, n, m, T, blk, wrm, dep, 9, default_warm(m), default_depth(m), dev)
    return _result(bits, T, s, s[0], s[0] / (n * T) if T else 0.0)


# ───────────────────────────── punctured captures ───────────────────────────

# Rows per output over the columns of a period ("101/110": row j, column c), for the code
# oct:171,133 with output 0 = X (ETSI EN 300 421, DVB-S)
PUNCTURE_PATTERNS = {
    "dvb:2/3": "10/11",
    "dvb:3/4": "101/110",
    "dvb:5/6": "10101/11010",
    "dvb:7/8": "1000101/1111010",
}
MAX_PERIOD = 16
# include/cvd.h CVD_VITERBI_PUNCT_WARM_GAIN, CVD_VITERBI_PUNCT_DEPTH_GAIN
PUNCT_WARM_GAIN = 2
PUNCT_DEPTH_GAIN = 5


def puncture_pattern(spec, n):
    """The column masks keep[c] of a puncturing pattern (bit j of keep[c]: output j of a step in
    column c is transmitted) from a list of masks, a string of rows per output ("101/110": row j,
    column c) or a name in PUNCTURE_PATTERNS.  1 <= period <= 16, every column nonzero."""
    n = int(n)
    if isinstance(spec, str):
        rows = PUNCTURE_PATTERNS.get(spec, spec).split("/")
        if len(rows) != n or len({len(r) for r in rows}) != 1 or any(set(r) - set("01") for r in rows):
            raise ValueError(f"puncture pattern {spec!r}: needs {n} rows of 0/1 of one length, or one of "
                             f"{sorted(PUNCTURE_PATTERNS)}")
        keep = [sum((rows[j][c] == "1") << j for j in range(n)) for c in range(len(rows[0]))]
    else:
        keep = [int(v) for v in spec]
    if not 1 <= len(keep) <= MAX_PERIOD:
        raise ValueError(f"puncture pattern: the period must be 1..{MAX_PERIOD}, not {len(keep)}")
    for v in keep:
        if v <= 0 or v >> n:
            raise ValueError(f"puncture pattern: column mask {v} must be nonzero and below 2^{n}")
    return keep


def punctured_bits(T, keep):
    """pos(T) - start of include/cvd.h: the capture bits that T steps of the pattern consume."""
    T = int(T)
    cnt = [bin(int(v)).count("1") for v in keep]
    return (T // len(cnt)) * sum(cnt) + sum(cnt[:T % len(cnt)])


def punctured_steps(bits, keep):
    """The largest T with punctured_bits(T, keep) <= bits."""
    cnt = [bin(int(v)).count("1") for v in keep]
    if bits <= 0:
        return 0
    T, left = (bits // sum(cnt)) * len(cnt), bits % sum(cnt)
    for c in cnt:
        if c > left:
            break
        left -= c
        T += 1
    return T


def default_warm_punctured(m, n, period, K):
    """include/cvd.h CVD_VITERBI_PUNCT_WARM."""
    return (default_warm(m) * (K + PUNCT_WARM_GAIN * (n * period - K)) + K - 1) // K


def default_depth_punctured(m, n, period, K):
    """include/cvd.h CVD_VITERBI_PUNCT_DEPTH."""
    return (default_depth(m) * (K + PUNCT_DEPTH_GAIN * (n * period - K)) + K - 1) // K


def decode_capture_punctured(n, m, gen, keep, capture, start=0, T=None, format="bytes", nbits=None, block=None,
                             warm=None, depth=None, device=None):
    """cvd_viterbi_decode_punctured: decode_capture over a capture that carries only the output
    bits that the puncturing pattern `keep` (anything puncture_pattern takes) transmits; the
    erased outputs do not count in the path distance.  Step t finds its kept bits at capture
    bit start + punctured_bits(t, keep).  T=None: as many steps as fit from `start`.  Returns
    decode_capture's dict with capture_bits = punctured_bits(T, keep) added and ber = errors /
    capture_bits; warm and depth default to default_warm_punctured / default_depth_punctured."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, start = int(n), int(m), int(start)
    code = as_code(gen, m, 1, n)
    keep = puncture_pattern(keep, n)
    period, K = len(keep), punctured_bits(len(keep), keep)
    cap, fmt, nbits = capture_buffer(capture, format, nbits, dev)
    if T is None:
        T = punctured_steps(nbits - start, keep) if start >= 0 else 0
    T, blk, wrm, dep = _steps(T, block, warm, depth)
    bits, s = _decode("decode_capture_punctured", "cvd_viterbi_decode_punctured", "cvd_viterbi_workspace_bytes",
                      (code.c, bytes(keep), period), (fmt,), cap, nbits, start, n, m, T, blk, wrm, dep, 10,
                      default_warm_punctured(m, n, period, K), default_depth_punctured(m, n, period, K), dev)
    res = _result(bits, T, s, s[0], s[0] / s[9] if T else 0.0)
    res["capture_bits"] = int(s[9])
    return res


def sync_punctured(n, m, gen, keep, capture, start=0, T=1000, format="bytes", nbits=None, block=None, warm=None,
                   depth=None, device=None):
    """Where do the puncturing periods begin?  Runs decode_capture_punctured over the first T
    steps from each of the K bit offsets of a period (K = the capture bits of one period): from
    capture bit start + o, o = 0..K-1.  Returns the K result dicts, each with `offset`, ranked
    by (errors ascending, offset ascending): the path distance is small at the right offset and
    large elsewhere.  K decoder calls, no kernel of its own.
    Some patterns make a code catastrophic, or leave several offsets indistinguishable; the list
    then shows near-equal error counts.  What the ranking means is the caller's reading, not a
    verdict of this function."""
    keep = puncture_pattern(keep, n)
    res = []
    for o in range(punctured_bits(len(keep), keep)):
        r = decode_capture_punctured(n, m, gen, keep, capture, start=int(start) + o, T=T, format=format, nbits=nbits,
                                     block=block, warm=warm, depth=depth, device=device)
        r["offset"] = o
        res.append(r)
    return sorted(res, key=lambda r: (r["errors"], r["offset"]))


# ───────────────────────────── soft decisions ───────────────────────────────

def soft_from_bits(bits, amplitude=1):
    """Hard bits as a soft capture: 0 -> -amplitude, 1 -> +amplitude (int8), 1 <= amplitude <= 127."""
    amplitude = int(amplitude)
    if not 1 <= amplitude <= 127:
        raise ValueError(f"amplitude = {amplitude}: must be 1..127")
    if isinstance(bits, torch.Tensor):
        if bool(((bits != 0) & (bits != 1)).any()):
            raise ValueError("soft_from_bits takes bits: 0 or 1")
        return ((2 * bits.to(torch.int16) - 1) * amplitude).to(torch.int8)
    b = np.asarray(bits)
    if ((b != 0) & (b != 1)).any():
        raise ValueError("soft_from_bits takes bits: 0 or 1")
    return ((2 * b.astype(np.int16) - 1) * amplitude).astype(np.int8)


def _soft_buffer(soft, device):
    """(device int8 tensor readable to a multiple of 16 bytes, number of values) of a soft capture
    given as a numpy array or torch tensor of int8: capture_buffer's rule for its uploads."""
    if isinstance(soft, np.ndarray):
        soft = np.ascontiguousarray(soft)
        soft = torch.from_numpy(soft if soft.flags.writeable else soft.copy())
    cap = soft
    if not isinstance(cap, torch.Tensor) or cap.dtype != torch.int8:
        raise TypeError("a soft capture is a numpy array or torch tensor of int8")
    cap = cap.reshape(-1)
    nvals = cap.numel()
    if cap.device != device or not cap.is_contiguous() or nvals % 16 or cap.data_ptr() % 16:
        buf = torch.zeros((nvals + 15) // 16 * 16 or 16, dtype=torch.int8, device=device)
        buf[:nvals].copy_(cap)
        cap = buf
    return cap, nvals


def _depuncture(L, cap, nvals, start, keep, n, T, dev):
    """cvd_soft_depuncture into a fresh buffer of n T values rounded up to 16 bytes."""
    out = torch.empty((n * T + 15) // 16 * 16 or 16, dtype=torch.int8, device=dev)
    _lib.check(L.cvd_soft_depuncture(ctypes.c_void_p(cap.data_ptr()), nvals, start, bytes(keep), len(keep), n, T,
                                     ctypes.c_void_p(out.data_ptr()), _stream_ptr()))
    return out


def depuncture_soft(soft, keep, n, start=0, T=None, device=None):
    """cvd_soft_depuncture: the punctured soft capture `soft` (int8) from value `start` spread out
    to n values per step, zeros (erasures) where the pattern `keep` (anything puncture_pattern
    takes) transmits nothing.  T=None: as many steps as fit.  Returns a device int8 tensor of
    n T values (a view of a buffer padded with zeros to 16 bytes: decode_capture_soft uses it in
    place)."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, start = int(n), int(start)
    keep = puncture_pattern(keep, n)
    cap, nvals = _soft_buffer(soft, dev)
    if T is None:
        T = punctured_steps(nvals - start, keep) if start >= 0 else 0
    T = int(T)
    with torch.cuda.device(dev):
        out = _depuncture(_lib.lib(), cap, nvals, start, keep, n, T, dev)
        torch.cuda.current_stream().synchronize()        # cap may be freed on return
    return out[:n * max(T, 0)]


def decode_capture_soft(n, m, gen, soft, start=0, T=None, keep=None, block=None, warm=None, depth=None, device=None):
    """cvd_viterbi_decode_soft over a soft capture (numpy array or torch tensor of int8: v > 0
    says 1, v < 0 says 0, 0 is an erasure, |v| the confidence): value start + n*t + j belongs to
    output j of step t.  T=None: as many whole steps as fit from `start`.  Returns
    decode_capture's dict with metric (the soft distance of the decoded path) and erasures added;
    errors counts the values whose sign disagrees with the path and ber = errors / (n T -
    erasures) (0.0 when nothing is left).
    keep (anything puncture_pattern takes): the capture is punctured, step t finds its kept
    values at start + punctured_bits(t, keep); it is depunctured on the device
    (cvd_soft_depuncture: zeros where nothing was sent) and decoded by the same call.  T=None
    then means as many steps as fit, warm and depth default to default_warm_punctured /
    default_depth_punctured, and capture_bits = punctured_bits(T, keep) is added."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, start = int(n), int(m), int(start)
    code = as_code(gen, m, 1, n)
    if keep is not None:
        keep = puncture_pattern(keep, n)
    cap, nvals = _soft_buffer(soft, dev)
    if T is None:
        fit = max(0, nvals - start) if start >= 0 else 0
        T = fit // n if keep is None else punctured_steps(fit, keep)
    T, blk, wrm, dep = _steps(T, block, warm, depth)
    prepare = None
    if keep is not None:
        period, K = len(keep), punctured_bits(len(keep), keep)
        if wrm < 0:
            wrm = default_warm_punctured(m, n, period, K)
        if dep < 0:
            dep = default_depth_punctured(m, n, period, K)
        # validates the pattern's range; T == 0: no launch
        prepare = lambda L: (_depuncture(L, cap, nvals, start, keep, n, T, dev), n * T, 0)
    bits, s = _decode("decode_capture_soft", "cvd_viterbi_decode_soft", "cvd_viterbi_soft_workspace_bytes", (code.c,), (),
                      cap, nvals, start, n, m, T, blk, wrm, dep, 11, default_warm(m), default_depth(m), dev, prepare)
    res = _result(bits, T, s, s[9], s[9] / s[10] if s[10] else 0.0)
    res.update(metric=int(s[0]), erasures=n * T - int(s[10]))
    if keep is not None:
        res["capture_bits"] = punctured_bits(T, keep)
    return res


def sync_punctured_soft(n, m, gen, keep, soft, start=0, T=1000, block=None, warm=None, depth=None, device=None):
    """sync_punctured over a soft capture: decode_capture_soft(keep=...) over the first T steps
    from each of the K value offsets of a period, the K result dicts, each with `offset`, ranked
    by (metric ascending, offset ascending).  What the ranking means is the caller's reading, as
    there."""
    keep = puncture_pattern(keep, n)
    res = []
    for o in range(punctured_bits(len(keep), keep)):
        r = decode_capture_soft(n, m, gen, soft, start=int(start) + o, T=T, keep=keep, block=block, warm=warm,
                                depth=depth, device=device)
        r["offset"] = o
        res.append(r)
    return sorted(res, key=lambda r: (r["metric"], r["offset"]))


# ───────────────────────────── framed captures ──────────────────────────────

FRAME_MAX_T = 65536      # include/cvd.h CVD_VITERBI_FRAME_MAX_T
FRAME_ANY = -1           # include/cvd.h CVD_FRAME_ANY


def _frame_state(name, s, m):
    """A boundary state as the library takes it: None is CVD_FRAME_ANY."""
    if s is None:
        return FRAME_ANY
    s = int(s)
    if not 0 <= s < (1 << m):
        raise ValueError(f"{name} = {s}: a state in [0, {1 << m}), or None for any")
    return s


def _frame_placement(nbits, span, w, F, start, stride, offsets, dev):
    """Where the frames of `span` capture positions lie: (offsets on the device or None, F, start,
    stride) as the library's frame calls take them."""
    off = None
    if offsets is not None:
        off = torch.from_numpy(np.ascontiguousarray(offsets)) if isinstance(offsets, np.ndarray) else offsets
        if not isinstance(off, torch.Tensor) or off.dtype != torch.int64:
            raise TypeError("offsets is a numpy array or torch tensor of int64")
        off = off.reshape(-1).to(dev).contiguous()
        if F is not None and int(F) != off.numel():
            raise ValueError(f"F = {F} but {off.numel()} offsets")
        F, start, stride = off.numel(), 0, 1
    else:
        start = int(start)
        stride = span if stride is None else int(stride)
        if start < 0 or stride < 1:
            raise ValueError("needs start >= 0 and stride >= 1")
        fit = (nbits - start - span) // stride + 1 if nbits - start >= span else 0
        F = fit if F is None else int(F)
        if not 0 <= F <= fit:
            raise ValueError(f"F = {F}: {fit} frames of {span} capture positions fit from {start} at stride {stride}")
    if F * w >= 1 << 31:
        raise ValueError(f"F = {F} frames of {w} words: the decoded bits must stay below 2^31 words")
    return off, F, start, stride


def _frames(who, entry, lead, fmt, cap, nbits, n, m, T, span, F, start, stride, offsets, start_state, end_state, soft,
            dev):
    """One call of the library's frame decoder `entry`(*lead, capture, nbits, *fmt, start, stride,
    offsets, F, T, start_state, end_state, bits, frames, stats, work, stream): decode_frames' dict.
    span: the capture bits (values) of a frame."""
    T = int(T)
    if not 1 <= T <= FRAME_MAX_T:
        raise ValueError(f"T = {T}: a frame has 1..{FRAME_MAX_T} steps")
    ss, es = _frame_state("start_state", start_state, m), _frame_state("end_state", end_state, m)
    if ss >= 0 and es >= 0 and T < m:
        raise ValueError(f"T = {T} < m = {m}: with both states fixed the end state is not reachable")
    w = (T + 31) // 32
    off, F, start, stride = _frame_placement(nbits, span, w, F, start, stride, offsets, dev)
    L = _lib.lib()
    call = getattr(L, entry)
    wbytes = int(L.cvd_viterbi_frames_workspace_bytes(n, m, T, F, int(soft)))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(call(*lead, None, 0, *fmt, 0, 1, None, 0, T, ss, es, None, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        bits = torch.empty((F, 4 * w), dtype=torch.uint8, device=dev)
        frames = torch.empty((F, 6), dtype=torch.int32, device=dev)
        s = [0, 0, 0, 0, 0, w]
        if F:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"{who}: the workspace of {F} frames of T = {T} steps (m = {m}) is {wbytes} bytes, "
                                  f"{free} bytes of device memory are free: decode the frames in pieces")
            stats = torch.zeros(6, dtype=torch.int64, device=dev)
            work = torch.empty(max(wbytes, 16), dtype=torch.uint8, device=dev)
            _lib.check(call(*lead, ctypes.c_void_p(cap.data_ptr()), nbits, *fmt, start, stride,
                            ctypes.c_void_p(off.data_ptr()) if off is not None else None, F, T, ss, es,
                            ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(frames.data_ptr()),
                            ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(work.data_ptr()), _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap, off and work may be freed on return
    return {"bits": bits, "frames": frames, "distance": frames[:, 0], "start_states": frames[:, 1],
            "end_states": frames[:, 2], "status": frames[:, 3], "errors": frames[:, 4], "counted": frames[:, 5],
            "T": T, "F": F, "decoded": int(s[1]), "skipped": int(s[2]), "total_distance": int(s[0]),
            "total_errors": int(s[3]), "total_counted": int(s[4]), "words": int(s[5]), "ber": s[3] / s[4] if s[4] else 0.0}


def decode_frames(n, m, gen, capture, T, F=None, start=0, stride=None, offsets=None, start_state=0, end_state=0,
                  keep=None, format="bytes", nbits=None, device=None):
    """cvd_viterbi_decode_frames: F frames of T steps each of the k = 1 code gen[j][i][d], decoded
    in one call.  Frame f begins at capture bit start + f*stride (stride=None: the frames follow
    one another, stride = the capture bits of a frame; F=None: as many frames as fit), or at
    offsets[f] (a numpy array or torch tensor of int64; a frame that does not lie inside the
    capture is skipped).  start_state / end_state: the state the encoder was in before / after
    the frame, None for unknown; the defaults are terminated frames (m zero tail bits).
    keep (anything puncture_pattern takes): the frames are punctured
    (cvd_viterbi_decode_frames_punctured), the pattern restarting at column 0 in every frame.
    Returns a dict: bits (device uint8 [F, 4w], w = ceil(T/32): row f LSB-packed), frames (device
    int32 [F, 6]) and the views of its columns distance, start_states, end_states, status (0
    decoded, 1 skipped), errors, counted; T, F, words (w), decoded, skipped, total_distance,
    total_errors, total_counted and ber = total_errors / total_counted."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    cap, fmt, nbits = capture_buffer(capture, format, nbits, dev)
    if keep is None:
        return _frames("decode_frames", "cvd_viterbi_decode_frames", (code.c,), (fmt,), cap, nbits, n, m, T, n * T, F,
                       start, stride, offsets, start_state, end_state, False, dev)
    keep = puncture_pattern(keep, n)
    return _frames("decode_frames", "cvd_viterbi_decode_frames_punctured", (code.c, bytes(keep), len(keep)), (fmt,), cap,
                   nbits, n, m, T, punctured_bits(max(T, 0), keep), F, start, stride, offsets, start_state, end_state,
                   False, dev)


def decode_frames_soft(n, m, gen, soft, T, F=None, start=0, stride=None, offsets=None, start_state=0, end_state=0,
                       keep=None, device=None):
    """cvd_viterbi_decode_frames_soft: decode_frames over a soft capture (int8, as
    decode_capture_soft takes it); start, stride and offsets count values.  distance is the soft
    distance of a frame's path, errors its sign disagreements, counted its non-erased values.
    Punctured soft frames have a call of their own: keep raises NotImplementedError (use
    decode_frames_soft_punctured)."""
    if keep is not None:
        raise NotImplementedError("decode_frames_soft takes no pattern: use decode_frames_soft_punctured")
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    cap, nvals = _soft_buffer(soft, dev)
    return _frames("decode_frames_soft", "cvd_viterbi_decode_frames_soft", (code.c,), (), cap, nvals, n, m, T, n * T, F,
                   start, stride, offsets, start_state, end_state, True, dev)


def decode_frames_soft_punctured(n, m, gen, keep, soft, T, F=None, start=0, stride=None, offsets=None, start_state=0,
                                 end_state=0, device=None):
    """cvd_viterbi_decode_frames_soft_punctured: decode_frames_soft over punctured frames (802.11a/g
    PPDUs at rates 2/3 and 3/4 as a demapper leaves them).  keep: anything puncture_pattern takes;
    the pattern restarts at column 0 in every frame, whose punctured_bits(T, keep) values follow
    one another from its offset.  The result is decode_frames_soft's on the frames depunctured
    one by one (zeros where nothing was sent), without that capture ever being built: counted is
    the number of kept values that are not 0."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    keep = puncture_pattern(keep, n)
    cap, nvals = _soft_buffer(soft, dev)
    return _frames("decode_frames_soft_punctured", "cvd_viterbi_decode_frames_soft_punctured",
                   (code.c, bytes(keep), len(keep)), (), cap, nvals, n, m, T, punctured_bits(max(T, 0), keep), F, start,
                   stride, offsets, start_state, end_state, True, dev)


# ──────────────────────────── tail-biting frames ────────────────────────────

TAILBITING_LAPS = 4      # include/cvd.h CVD_VITERBI_TAILBITING_LAPS
TAILBITING_MAX_LAPS = 8  # include/cvd.h CVD_VITERBI_TAILBITING_MAX_LAPS


def _tailbiting(who, entry, lead, fmt, cap, nbits, n, m, T, span, F, start, stride, offsets, max_laps, soft, dev):
    """One call of the library's tail-biting decoder `entry`(*lead, capture, nbits, *fmt, start,
    stride, offsets, F, T, max_laps, bits, frames, stats, work, stream): decode_frames_tailbiting's
    dict.  span: the capture bits (values) of a frame."""
    T = int(T)
    if not 1 <= T <= FRAME_MAX_T:
        raise ValueError(f"T = {T}: a frame has 1..{FRAME_MAX_T} steps")
    laps = 0 if max_laps is None else int(max_laps)
    if max_laps is not None and not 1 <= laps <= TAILBITING_MAX_LAPS:
        raise ValueError(f"max_laps = {max_laps}: 1..{TAILBITING_MAX_LAPS} laps, or None for {TAILBITING_LAPS}")
    w = (T + 31) // 32
    off, F, start, stride = _frame_placement(nbits, span, w, F, start, stride, offsets, dev)
    L = _lib.lib()
    call = getattr(L, entry)
    wbytes = int(L.cvd_viterbi_tailbiting_workspace_bytes(n, m, T, F, int(soft)))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(call(*lead, None, 0, *fmt, 0, 1, None, 0, T, laps, None, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        bits = torch.empty((F, 4 * w), dtype=torch.uint8, device=dev)
        frames = torch.empty((F, 8), dtype=torch.int32, device=dev)
        s = [0, 0, 0, 0, 0, w, 0, 0, 0]
        if F:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"{who}: the workspace of {F} frames of T = {T} steps (m = {m}) is {wbytes} bytes, "
                                  f"{free} bytes of device memory are free: decode the frames in pieces")
            stats = torch.zeros(9, dtype=torch.int64, device=dev)
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev) if wbytes else None
            _lib.check(call(*lead, ctypes.c_void_p(cap.data_ptr()), nbits, *fmt, start, stride,
                            ctypes.c_void_p(off.data_ptr()) if off is not None else None, F, T, laps,
                            ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(frames.data_ptr()),
                            ctypes.c_void_p(stats.data_ptr()),
                            ctypes.c_void_p(work.data_ptr()) if work is not None else None, _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap, off and work may be freed on return
    return {"bits": bits, "frames": frames, "distance": frames[:, 0], "start_states": frames[:, 1],
            "end_states": frames[:, 2], "status": frames[:, 3], "errors": frames[:, 4], "counted": frames[:, 5],
            "laps": frames[:, 6], "T": T, "F": F, "decoded": int(s[1]), "skipped": int(s[2]),
            "total_distance": int(s[0]), "total_errors": int(s[3]), "total_counted": int(s[4]), "words": int(s[5]),
            "fallback": int(s[6]), "open": int(s[7]), "total_laps": int(s[8]), "ber": s[3] / s[4] if s[4] else 0.0}


def decode_frames_tailbiting(n, m, gen, capture, T, F=None, start=0, stride=None, offsets=None, max_laps=None,
                             keep=None, format="bytes", nbits=None, device=None):
    """cvd_viterbi_decode_frames_tailbiting: F tail-biting frames of T steps each of the k = 1 code
    gen[j][i][d] (LTE PBCH / PDCCH, 802.16 FCH: the encoder starts in the state of the frame's own
    last m bits, so s_0 = s_T and neither is known), decoded in one call by the wrap-around Viterbi
    algorithm of include/cvd.h with at most max_laps laps (1..8; None: the library's default, 4).
    The frames are placed as decode_frames places them (start, stride, F, or offsets); keep: the
    frames are punctured (cvd_viterbi_decode_frames_tailbiting_punctured).
    Returns decode_frames' dict with frames a device int32 [F, 8] and its further column view laps;
    status is 0 (the best path is tail-biting), 2 (the best tail-biting survivor of the last lap),
    3 (no tail-biting survivor: s_0 != s_T) or 1 (skipped); the further totals fallback (frames of
    status 2), open (status 3) and total_laps; ber = total_errors / total_counted."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    cap, fmt, nbits = capture_buffer(capture, format, nbits, dev)
    if keep is None:
        return _tailbiting("decode_frames_tailbiting", "cvd_viterbi_decode_frames_tailbiting", (code.c,), (fmt,), cap,
                           nbits, n, m, T, n * T, F, start, stride, offsets, max_laps, False, dev)
    keep = puncture_pattern(keep, n)
    return _tailbiting("decode_frames_tailbiting", "cvd_viterbi_decode_frames_tailbiting_punctured",
                       (code.c, bytes(keep), len(keep)), (fmt,), cap, nbits, n, m, T, punctured_bits(max(T, 0), keep), F,
                       start, stride, offsets, max_laps, False, dev)


def decode_frames_tailbiting_soft(n, m, gen, soft, T, F=None, start=0, stride=None, offsets=None, max_laps=None,
                                  device=None):
    """cvd_viterbi_decode_frames_tailbiting_soft: decode_frames_tailbiting over a soft capture (int8,
    as decode_capture_soft takes it); start, stride and offsets count values.  distance is the soft
    distance of a frame's path, errors its sign disagreements, counted its non-erased values."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    cap, nvals = _soft_buffer(soft, dev)
    return _tailbiting("decode_frames_tailbiting_soft", "cvd_viterbi_decode_frames_tailbiting_soft", (code.c,), (), cap,
                       nvals, n, m, T, n * T, F, start, stride, offsets, max_laps, True, dev)


def decode_frames_tailbiting_soft_punctured(n, m, gen, keep, soft, T, F=None, start=0, stride=None, offsets=None,
                                            max_laps=None, device=None):
    """cvd_viterbi_decode_frames_tailbiting_soft_punctured: decode_frames_tailbiting_soft over
    punctured frames (802.16 FCH and bursts), the pattern `keep` restarting at column 0 in every
    frame and every lap.  The result is decode_frames_tailbiting_soft's on the frames depunctured
    one by one.  Python and C only: the command line does not reach it."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    keep = puncture_pattern(keep, n)
    cap, nvals = _soft_buffer(soft, dev)
    return _tailbiting("decode_frames_tailbiting_soft_punctured", "cvd_viterbi_decode_frames_tailbiting_soft_punctured",
                       (code.c, bytes(keep), len(keep)), (), cap, nvals, n, m, T, punctured_bits(max(T, 0), keep), F,
                       start, stride, offsets, max_laps, True, dev)


# ─────────────────────────── soft output per bit ────────────────────────────

LLR_SATURATED = 32767    # include/cvd.h: |L_t| of a step whose other input value has no path


def decode_frames_llr(n, m, gen, soft, T, F=None, start=0, stride=None, offsets=None, start_state=0, end_state=0,
                      device=None):
    """cvd_viterbi_decode_frames_llr: decode_frames_soft with a max-log-MAP value per bit.  The
    frames of the soft capture `soft` (int8, as decode_capture_soft takes it; hard bits go through
    soft_from_bits) are placed as decode_frames places them; start, stride and offsets count
    values.  L_t = (cost of the best path with u_t = 0) - (cost of the best path with u_t = 1),
    positive for a 1, in the units of the input; +-32767 where the other value has no path (the
    tail of a terminated frame).
    Returns a dict: llr (device int16 [F, T], a view of the rows padded to 32 w values), bits
    (device uint8 [F, 4w], w = ceil(T/32): bit t = [L_t > 0]), frames (device int32 [F, 6]) and the
    views of its columns distance (decode_frames_soft's), zeros (#{t : L_t = 0}), end_states,
    status (0 decoded, 1 skipped), weakest (min |L_t| over the unsaturated steps; 32767 if none),
    saturated (#{t : |L_t| = 32767}); T, F, words (w), decoded, skipped, total_distance,
    total_zeros and total_saturated."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    cap, nvals = _soft_buffer(soft, dev)
    return _llr("decode_frames_llr", "cvd_viterbi_decode_frames_llr", (code.c,), cap, nvals, n, m, T, n * T, F, start,
                stride, offsets, start_state, end_state, dev)


def decode_frames_llr_punctured(n, m, gen, keep, soft, T, F=None, start=0, stride=None, offsets=None, start_state=0,
                                end_state=0, device=None):
    """cvd_viterbi_decode_frames_llr_punctured: decode_frames_llr over punctured frames, the pattern
    `keep` (anything puncture_pattern takes) restarting at column 0 in every frame.  The result is
    decode_frames_llr's on the frames depunctured one by one (zeros where nothing was sent).
    Python and C only: the command line does not reach it."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T = int(n), int(m), int(T)
    code = as_code(gen, m, 1, n)
    keep = puncture_pattern(keep, n)
    cap, nvals = _soft_buffer(soft, dev)
    return _llr("decode_frames_llr_punctured", "cvd_viterbi_decode_frames_llr_punctured",
                (code.c, bytes(keep), len(keep)), cap, nvals, n, m, T, punctured_bits(max(T, 0), keep), F, start, stride,
                offsets, start_state, end_state, dev)


def _llr(who, entry, lead, cap, nvals, n, m, T, span, F, start, stride, offsets, start_state, end_state, dev):
    """One call of the library's soft-output decoder `entry`(*lead, soft, nvals, start, stride,
    offsets, F, T, start_state, end_state, llr, bits, frames, stats, work, stream):
    decode_frames_llr's dict.  span: the values of a frame."""
    if not 1 <= T <= FRAME_MAX_T:
        raise ValueError(f"T = {T}: a frame has 1..{FRAME_MAX_T} steps")
    ss, es = _frame_state("start_state", start_state, m), _frame_state("end_state", end_state, m)
    if ss >= 0 and es >= 0 and T < m:
        raise ValueError(f"T = {T} < m = {m}: with both states fixed the end state is not reachable")
    w = (T + 31) // 32
    off, F, start, stride = _frame_placement(nvals, span, w, F, start, stride, offsets, dev)
    L = _lib.lib()
    call = getattr(L, entry)
    wbytes = int(L.cvd_viterbi_llr_workspace_bytes(n, m, T, F))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(call(*lead, None, 0, 0, 1, None, 0, T, ss, es, None, None, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        llr = torch.empty((F, 32 * w), dtype=torch.int16, device=dev)
        bits = torch.empty((F, 4 * w), dtype=torch.uint8, device=dev)
        frames = torch.empty((F, 6), dtype=torch.int32, device=dev)
        s = [0, 0, 0, 0, 0, w]
        if F:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"{who}: the workspace of {F} frames of T = {T} steps (m = {m}) is "
                                  f"{wbytes} bytes, {free} bytes of device memory are free: decode the frames in pieces")
            stats = torch.zeros(6, dtype=torch.int64, device=dev)
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev) if wbytes else None
            _lib.check(call(*lead, ctypes.c_void_p(cap.data_ptr()), nvals, start, stride,
                            ctypes.c_void_p(off.data_ptr()) if off is not None else None, F, T, ss, es,
                            ctypes.c_void_p(llr.data_ptr()), ctypes.c_void_p(bits.data_ptr()),
                            ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                            ctypes.c_void_p(work.data_ptr()) if work is not None else None, _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap, off and work may be freed on return
    return {"llr": llr[:, :T], "bits": bits, "frames": frames, "distance": frames[:, 0], "zeros": frames[:, 1],
            "end_states": frames[:, 2], "status": frames[:, 3], "weakest": frames[:, 4], "saturated": frames[:, 5],
            "T": T, "F": F, "decoded": int(s[1]), "skipped": int(s[2]), "total_distance": int(s[0]),
            "total_zeros": int(s[3]), "total_saturated": int(s[4]), "words": int(s[5])}


# ───────────────────────── list decoding and the CRC ────────────────────────

LIST_MAX_L = 8           # include/cvd.h CVD_VITERBI_LIST_MAX_L
LIST_MAX_T = 8192        # include/cvd.h CVD_VITERBI_LIST_MAX_T

CRC_SPECS = {            # name: (width, poly, init, expect)
    "crc8-lte": (8, 0x9B, 0, 0),
    "crc16-ccitt": (16, 0x1021, 0, 0),
    "crc24a": (24, 0x864CFB, 0, 0),
    "crc24b": (24, 0x800063, 0, 0),
    "crc32": (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF),
}


def crc_spec(spec):
    """(width, poly, init, expect) of a name in CRC_SPECS, of "WIDTH:POLY[:INIT[:EXPECT]]" (the
    width decimal, the others hexadecimal; init and expect default to 0), or of such a tuple.
    width is 1..32 and the others are below 2^width."""
    if isinstance(spec, str):
        if spec in CRC_SPECS:
            return CRC_SPECS[spec]
        parts = spec.split(":")
        try:
            if not 2 <= len(parts) <= 4:
                raise ValueError
            vals = [int(parts[0], 10)] + [int(p, 16) for p in parts[1:]]
        except ValueError:
            raise ValueError(f"CRC {spec!r}: WIDTH:POLY[:INIT[:EXPECT]] with the width decimal and the others "
                             f"hexadecimal, or one of {sorted(CRC_SPECS)}") from None
        vals += [0] * (4 - len(vals))
    else:
        vals = [int(v) for v in spec]
        if len(vals) != 4:
            raise ValueError("a CRC is (width, poly, init, expect)")
    width, poly, init, expect = vals
    if not 1 <= width <= 32:
        raise ValueError(f"CRC {spec!r}: the width must be 1..32")
    if any(v < 0 or v >> width for v in (poly, init, expect)):
        raise ValueError(f"CRC {spec!r}: poly, init and expect must be below 2^{width}")
    return width, poly, init, expect


def _list_call(who, code, cap, nvals, n, m, T, L, F, start, stride, offsets, start_state, end_state, dev):
    """One call of cvd_viterbi_decode_frames_list: (bits [F, L, 4w], paths [F, L, 3], frames [F, 2],
    the five stats, F)."""
    if not 1 <= T <= LIST_MAX_T:
        raise ValueError(f"T = {T}: a frame of the list decoder has 1..{LIST_MAX_T} steps")
    if not 1 <= L <= LIST_MAX_L:
        raise ValueError(f"L = {L}: the list holds 1..{LIST_MAX_L} paths")
    ss, es = _frame_state("start_state", start_state, m), _frame_state("end_state", end_state, m)
    if ss >= 0 and es >= 0 and T < m:
        raise ValueError(f"T = {T} < m = {m}: with both states fixed the end state is not reachable")
    w = (T + 31) // 32
    off, F, start, stride = _frame_placement(nvals, n * T, L * w, F, start, stride, offsets, dev)
    lib = _lib.lib()
    call = lib.cvd_viterbi_decode_frames_list
    wbytes = int(lib.cvd_viterbi_list_workspace_bytes(n, m, T, F, L))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(call(code.c, None, 0, 0, 1, None, 0, T, ss, es, L, None, None, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        bits = torch.empty((F, L, 4 * w), dtype=torch.uint8, device=dev)
        paths = torch.empty((F, L, 3), dtype=torch.int32, device=dev)
        frames = torch.empty((F, 2), dtype=torch.int32, device=dev)
        s = [0, 0, 0, 0, w]
        if F:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"{who}: the workspace of {F} frames of T = {T} steps (m = {m}, L = {L}) is "
                                  f"{wbytes} bytes, {free} bytes of device memory are free: decode the frames in pieces")
            stats = torch.zeros(5, dtype=torch.int64, device=dev)
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev) if wbytes else None
            _lib.check(call(code.c, ctypes.c_void_p(cap.data_ptr()), nvals, start, stride,
                            ctypes.c_void_p(off.data_ptr()) if off is not None else None, F, T, ss, es, L,
                            ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(paths.data_ptr()),
                            ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                            ctypes.c_void_p(work.data_ptr()) if work is not None else None, _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap, off and work may be freed on return
    return bits, paths, frames, s, F


def decode_frames_list(n, m, gen, soft, T, L, F=None, start=0, stride=None, offsets=None, start_state=0, end_state=0,
                       device=None):
    """cvd_viterbi_decode_frames_list: decode_frames_soft returning the L best paths of every frame
    (the parallel list Viterbi algorithm), 1 <= L <= 8, 1 <= T <= 8192.  The frames of the soft
    capture `soft` (int8) are placed as decode_frames places them; start, stride and offsets count
    values.  Path 0 is decode_frames_soft's; distances do not decrease along the list.
    Returns a dict: bits (device uint8 [F, L, 4w], w = ceil(T/32): row (f, l) is path l of frame f,
    LSB-packed, zero where the path is absent), distance, start_states, end_states (device int32
    [F, L]; -1 where absent), paths (device int32 [F]: how many were found) and status (0 decoded,
    1 skipped); total_distance (of the paths 0), decoded, skipped, total_paths, words (w), T, F, L."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T, L = int(n), int(m), int(T), int(L)
    code = as_code(gen, m, 1, n)
    cap, nvals = _soft_buffer(soft, dev)
    bits, paths, frames, s, F = _list_call("decode_frames_list", code, cap, nvals, n, m, T, L, F, start, stride, offsets,
                                           start_state, end_state, dev)
    return {"bits": bits, "distance": paths[:, :, 0], "start_states": paths[:, :, 1], "end_states": paths[:, :, 2],
            "paths": frames[:, 0], "status": frames[:, 1], "total_distance": int(s[0]), "decoded": int(s[1]),
            "skipped": int(s[2]), "total_paths": int(s[3]), "words": int(s[4]), "T": T, "F": F, "L": L}


def frames_crc(bits, first, count, spec, device=None):
    """cvd_frames_crc over rows of decoded bits: `bits` is uint8 [..., 4w] (a device tensor or a
    numpy array; any layout that the frame decoders write: bit t of a row is bit t & 7 of byte
    t >> 3), the CRC `spec` (anything crc_spec takes) runs over the `count` bits from bit `first` of
    every row and is compared with the width bits that follow, the first of them most significant.
    Returns the values register ^ field as an int64 tensor in 0..2^32 - 1 of the leading shape: 0
    where an appended CRC matches (crc_spec's `expect` in general)."""
    width, poly, init, _ = crc_spec(spec)
    first, count = int(first), int(count)
    if isinstance(bits, np.ndarray):
        bits = torch.from_numpy(np.ascontiguousarray(bits))
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.uint8 or bits.dim() < 1 or bits.shape[-1] % 4 \
            or bits.shape[-1] == 0:
        raise TypeError("rows of bits are a numpy array or torch tensor of uint8 [..., 4w]")
    if first < 0 or count < 0 or first + count + width > 8 * bits.shape[-1]:
        raise ValueError(f"first = {first}, count = {count}: the data and the {width} bits behind them must lie "
                         f"inside the {8 * bits.shape[-1]} bits of a row")
    if bits.is_cuda and device is None:
        dev = bits.device
    else:
        dev = device if isinstance(device, torch.device) else _require_gpu(device)
    lead, w = bits.shape[:-1], bits.shape[-1] // 4
    rows = int(np.prod(lead, dtype=np.int64))
    with torch.cuda.device(dev):
        buf = bits.to(dev).contiguous()
        if buf.data_ptr() % 4:
            buf = buf.clone()
        value = torch.zeros(max(rows, 1), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().cvd_frames_crc(ctypes.c_void_p(buf.data_ptr()) if rows else None, rows, w, first, count,
                                             width, poly, init, ctypes.c_void_p(value.data_ptr()), _stream_ptr()))
        out = (value[:rows].to(torch.int64) & 0xFFFFFFFF).reshape(lead)
        torch.cuda.current_stream().synchronize()        # buf may be freed on return
    return out


def decode_frames_crc(n, m, gen, soft, T, L, crc, first=0, count=None, expect=None, F=None, start=0, stride=None,
                      offsets=None, start_state=0, end_state=0, device=None):
    """decode_frames_list and the CRC `crc` (anything crc_spec takes) over all F L rows on the
    device: of every frame the first path of the list that passes the check.  The CRC runs over
    `count` bits from bit `first` (count=None: T - first - width - (m if end_state is fixed else 0), a frame
    of data || CRC || tail) and a path passes when its value equals `expect` (None: the spec's).
    Returns decode_frames_list's dict and: value (device int64 [F, L]), choice (device int32 [F]: the
    lowest present l whose value equals expect, -1 if none), crc_ok (device bool [F]), chosen_bits
    (device uint8 [F, 4w]: the chosen row, path 0 where none passes), chosen_distance (device int32
    [F]), and the totals ok (frames with crc_ok) and rescued (frames with choice > 0)."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T, L = int(n), int(m), int(T), int(L)
    width, poly, init, exp0 = crc_spec(crc)
    expect = exp0 if expect is None else int(expect)
    if expect < 0 or expect >> width:
        raise ValueError(f"expect = {expect}: a value below 2^{width}")
    first = int(first)
    if count is None:
        count = T - width - first - (m if end_state is not None else 0)
    count = int(count)
    if first < 0 or count < 0 or first + count + width > T:
        raise ValueError(f"first = {first}, count = {count}: the data and the {width} CRC bits must lie inside the "
                         f"{T} bits of a frame")
    res = decode_frames_list(n, m, gen, soft, T, L, F=F, start=start, stride=stride, offsets=offsets,
                             start_state=start_state, end_state=end_state, device=dev)
    F = res["F"]
    with torch.cuda.device(dev):
        value = frames_crc(res["bits"], first, count, (width, poly, init, expect), device=dev)
        present = torch.arange(L, device=dev)[None, :] < res["paths"][:, None]
        hit = (value == expect) & present
        ok = hit.any(dim=1)
        choice = torch.where(ok, hit.to(torch.int32).argmax(dim=1), torch.full_like(res["paths"], -1, dtype=torch.int64))
        pick = choice.clamp(min=0)
        rows = torch.arange(F, device=dev)
        res.update(value=value, choice=choice.to(torch.int32), crc_ok=ok, chosen_bits=res["bits"][rows, pick],
                   chosen_distance=res["distance"][rows, pick], ok=int(ok.sum()), rescued=int((choice > 0).sum()))
    return res


# ─────────────────── list decoding of tail-biting frames ────────────────────

def decode_frames_tailbiting_list(n, m, gen, soft, T, L, F=None, start=0, stride=None, offsets=None, max_laps=None,
                                  device=None):
    """cvd_viterbi_decode_frames_tailbiting_list: decode_frames_tailbiting_soft returning up to L
    paths of every frame, 1 <= L <= 8, 1 <= T <= 8192: path 0 is decode_frames_tailbiting_soft's,
    paths 1.. are the cheapest tail-biting entries (s_0 = s_T) of the last lap's end lists, in
    ascending order of their distance (one of them may be cheaper than a path 0 of status 2 or 3).
    The frames of the soft capture `soft` (int8) are placed as decode_frames places them; start,
    stride and offsets count values; max_laps as in decode_frames_tailbiting (1..8; None: 4).
    The result for L is not the first L paths of the result for a larger L.
    Returns a dict: bits (device uint8 [F, L, 4w], w = ceil(T/32): row (f, l) is path l of frame f,
    LSB-packed, zero where the path is absent), distance, start_states, end_states (device int32
    [F, L]; -1 where absent), frames (device int32 [F, 4]) and the views of its columns paths (how
    many were found), status (0, 2, 3 as decode_frames_tailbiting; 1 skipped), laps and candidates
    (the tail-biting entries of the last lap, |C|); total_distance (of the paths 0), decoded,
    skipped, total_paths, words (w), fallback (frames of status 2), open (status 3), total_laps, T,
    F, L.  Python and C only: the command line does not reach it."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T, L = int(n), int(m), int(T), int(L)
    code = as_code(gen, m, 1, n)
    cap, nvals = _soft_buffer(soft, dev)
    if not 1 <= T <= LIST_MAX_T:
        raise ValueError(f"T = {T}: a frame of the list decoder has 1..{LIST_MAX_T} steps")
    if not 1 <= L <= LIST_MAX_L:
        raise ValueError(f"L = {L}: the list holds 1..{LIST_MAX_L} paths")
    laps = 0 if max_laps is None else int(max_laps)
    if max_laps is not None and not 1 <= laps <= TAILBITING_MAX_LAPS:
        raise ValueError(f"max_laps = {max_laps}: 1..{TAILBITING_MAX_LAPS} laps, or None for {TAILBITING_LAPS}")
    w = (T + 31) // 32
    off, F, start, stride = _frame_placement(nvals, n * T, L * w, F, start, stride, offsets, dev)
    lib = _lib.lib()
    call = lib.cvd_viterbi_decode_frames_tailbiting_list
    wbytes = int(lib.cvd_viterbi_tailbiting_list_workspace_bytes(n, m, T, F, L))
    if wbytes < 0:
        # the decoder itself names an unsupported code shape
        _lib.check(call(code.c, None, 0, 0, 1, None, 0, T, laps, L, None, None, None, None, None, None))
        _lib.check(wbytes)
    with torch.cuda.device(dev):
        bits = torch.empty((F, L, 4 * w), dtype=torch.uint8, device=dev)
        paths = torch.empty((F, L, 3), dtype=torch.int32, device=dev)
        frames = torch.empty((F, 4), dtype=torch.int32, device=dev)
        s = [0, 0, 0, 0, w, 0, 0, 0]
        if F:
            free = torch.cuda.mem_get_info(dev)[0]
            if wbytes > free:
                raise MemoryError(f"decode_frames_tailbiting_list: the workspace of {F} frames of T = {T} steps (m = {m}, "
                                  f"L = {L}) is {wbytes} bytes, {free} bytes of device memory are free: decode the "
                                  f"frames in pieces")
            stats = torch.zeros(8, dtype=torch.int64, device=dev)
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev) if wbytes else None
            _lib.check(call(code.c, ctypes.c_void_p(cap.data_ptr()), nvals, start, stride,
                            ctypes.c_void_p(off.data_ptr()) if off is not None else None, F, T, laps, L,
                            ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(paths.data_ptr()),
                            ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(stats.data_ptr()),
                            ctypes.c_void_p(work.data_ptr()) if work is not None else None, _stream_ptr()))
            s = stats.cpu().tolist()     # synchronises: cap, off and work may be freed on return
    return {"bits": bits, "distance": paths[:, :, 0], "start_states": paths[:, :, 1], "end_states": paths[:, :, 2],
            "frames": frames, "paths": frames[:, 0], "status": frames[:, 1], "laps": frames[:, 2],
            "candidates": frames[:, 3], "total_distance": int(s[0]), "decoded": int(s[1]), "skipped": int(s[2]),
            "total_paths": int(s[3]), "words": int(s[4]), "fallback": int(s[5]), "open": int(s[6]),
            "total_laps": int(s[7]), "T": T, "F": F, "L": L}


def decode_frames_tailbiting_crc(n, m, gen, soft, T, L, crc, first=0, count=None, expect=None, F=None, start=0,
                                 stride=None, offsets=None, max_laps=None, device=None):
    """decode_frames_tailbiting_list and the CRC `crc` (anything crc_spec takes) over all F L rows
    on the device: of every frame the first path of the list that passes the check (LTE PBCH and
    PDCCH, 802.16 FCH, EDGE control blocks: short tail-biting frames that end in a CRC).  The CRC
    runs over `count` bits from bit `first` (count=None: T - first - width, a frame of data || CRC)
    and a path passes when its value equals `expect` (None: the spec's).  Where the CRC is masked
    with an identity (the RNTI of an LTE DCI) and the identity is known, pass it as `expect`; where
    it is not, leave expect=None and read the identity out of `value`: value[f, l] is register ^
    field of path l, which is the mask that the sender applied if the path is the sent one (choice,
    crc_ok and rescued then only mark the paths whose mask is the spec's own `expect`).
    Returns decode_frames_tailbiting_list's dict and: value (device int64 [F, L]), choice (device
    int32 [F]: the lowest present l whose value equals expect, -1 if none), crc_ok (device bool
    [F]), chosen_bits (device uint8 [F, 4w]: the chosen row, path 0 where none passes),
    chosen_distance (device int32 [F]), and the totals ok (frames with crc_ok) and rescued (frames
    with choice > 0)."""
    dev = device if isinstance(device, torch.device) else _require_gpu(device)
    n, m, T, L = int(n), int(m), int(T), int(L)
    width, poly, init, exp0 = crc_spec(crc)
    expect = exp0 if expect is None else int(expect)
    if expect < 0 or expect >> width:
        raise ValueError(f"expect = {expect}: a value below 2^{width}")
    first = int(first)
    count = T - width - first if count is None else int(count)
    if first < 0 or count < 0 or first + count + width > T:
        raise ValueError(f"first = {first}, count = {count}: the data and the {width} CRC bits must lie inside the "
                         f"{T} bits of a frame")
    res = decode_frames_tailbiting_list(n, m, gen, soft, T, L, F=F, start=start, stride=stride, offsets=offsets,
                                        max_laps=max_laps, device=dev)
    F = res["F"]
    with torch.cuda.device(dev):
        value = frames_crc(res["bits"], first, count, (width, poly, init, expect), device=dev)
        present = torch.arange(L, device=dev)[None, :] < res["paths"][:, None]
        hit = (value == expect) & present
        ok = hit.any(dim=1)
        choice = torch.where(ok, hit.to(torch.int32).argmax(dim=1), torch.full_like(res["paths"], -1, dtype=torch.int64))
        pick = choice.clamp(min=0)
        rows = torch.arange(F, device=dev)
        res.update(value=value, choice=choice.to(torch.int32), crc_ok=ok, chosen_bits=res["bits"][rows, pick],
                   chosen_distance=res["distance"][rows, pick], ok=int(ok.sum()), rescued=int((choice > 0).sum()))
    return res

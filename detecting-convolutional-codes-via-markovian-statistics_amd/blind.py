"""Blind parity-check search of a captured bitstream (nothing in the reference, whose
templates all come from known generators): which convolutional code is in this capture,
and at which symbol phase?

For a span of s delays a B = n*(s+1)-bit word slides over the capture one symbol at a
time; one histogram of the words and one Walsh-Hadamard transform give the satisfaction
count of all 2^B parity templates at once (cvd_parity_sweep, include/cvd.h; HIP kernels in
csrc/cvd_sweep.hip).  The code's parity checks are the masks whose count is far from T/2;
for k = 1, n = 2 the shortest one is the generator pair itself.  Integer arithmetic up to
the ranking: the same capture always gives the same list.  No CPU fallback.

Masks and templates: bit n*e + j of a word is output j of symbol a + e, and the template
term (output j, delay s) of parity.py is mask bit n*(span - s) + j.
"""
import ctypes
import math

import torch

from . import _lib
from .detector import _require_gpu, _stream_ptr, capture_buffer

MAX_T = (1 << 31) - 1    # anchors per cvd_parity_sweep call (include/cvd.h)


def _device(device):
    return device if isinstance(device, torch.device) else _require_gpu(device)


def _bits(n, span):
    n, span = int(n), int(span)
    if not 1 <= n <= 3 or span < 0:
        raise ValueError(f"needs n in 1..3 and span >= 0, not n = {n}, span = {span}")
    return n * (span + 1)


def template_mask(template, n, span):
    """Mask of a template [(output j, delay s), ...] over a window of span + 1 symbols."""
    _bits(n, span)
    mask = 0
    for j, s in template:
        j, s = int(j), int(s)
        if not 0 <= j < n:
            raise ValueError(f"output {j} outside 0..{n - 1}")
        if not 0 <= s <= span:
            raise ValueError(f"delay {s} outside the span 0..{span}")
        mask ^= 1 << (n * (span - s) + j)
    return mask


def mask_template(mask, n, span):
    """The template of a mask, in template_of's order (by output, then delay): the
    inverse of template_mask."""
    B = _bits(n, span)
    mask = int(mask)
    if not 0 <= mask < 1 << B:
        raise ValueError(f"mask {mask:#x} outside the window's {B} bits")
    return sorted((b % n, span - b // n) for b in range(B) if (mask >> b) & 1)


def mask_extent(mask, n):
    """Symbols from a mask's lowest to its highest set bit."""
    mask = int(mask)
    return (mask.bit_length() - 1) // n - ((mask & -mask).bit_length() - 1) // n + 1


def anchors_in(nbits, n, span, start=0, n_phase=1):
    """Anchors T for which every word of every phase lies inside capture bits [start, nbits)."""
    room = int(nbits) - int(start) - (int(n_phase) - 1) - _bits(n, span)
    return room // int(n) + 1 if room >= 0 else 0


def parity_sweep(capture, n, span, start=0, T=None, n_phase=1, format="bytes", nbits=None, device=None):
    """cvd_parity_sweep over a capture (numpy array or torch tensor of uint8, as
    Detector.pack_capture takes it): the int64 tensor [n_phase, 2^B] on the device with
    sat[f][mask] = #{anchors a < T of phase f whose word satisfies the mask}, word bit i =
    capture bit start + f + n*a + i.  T=None: as many anchors as fit; a T above 2^31 - 1 is
    split into calls that accumulate."""
    dev = _device(device)
    B = _bits(n, span)
    cap, fmt, nbits = capture_buffer(capture, format, nbits, dev)
    n, span, start, n_phase = int(n), int(span), int(start), int(n_phase)
    L = _lib.lib()
    wbytes = int(L.cvd_parity_sweep_workspace_bytes(n, span, n_phase))
    if wbytes < 0:
        _lib.check(wbytes)
    T = anchors_in(nbits, n, span, start, n_phase) if T is None else int(T)
    if T < 0:
        raise ValueError("T must be >= 0")
    with torch.cuda.device(dev):
        sat = torch.zeros((n_phase, 1 << B), dtype=torch.int64, device=dev)
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        for a0 in range(0, T, MAX_T):
            _lib.check(L.cvd_parity_sweep(ctypes.c_void_p(cap.data_ptr()), nbits, fmt, n, span, start + n * a0,
                                          min(MAX_T, T - a0), n_phase, ctypes.c_void_p(sat.data_ptr()),
                                          ctypes.c_void_p(work.data_ptr()), _stream_ptr()))
        torch.cuda.current_stream().synchronize()   # cap and work may be freed on return
    return sat


def default_z_min(n_phase, B):
    """sqrt(2 ln(n_phase 2^B)) + 3: three sigma above the level the largest of n_phase*2^B
    unbiased masks reaches."""
    return math.sqrt(2.0 * math.log(n_phase * 2.0 ** B)) + 3.0


def find_parity_checks(capture, n, max_span, start=0, T=None, format="bytes", nbits=None, z_min=None, top=16,
                       device=None):
    """The parity checks a capture satisfies: one sweep at max_span over all n symbol
    phases, then every mask != 0 with (2 sat - T)^2 >= z_min^2 T (default z_min:
    default_z_min), ranked by extent (symbols from the lowest to the highest set bit)
    ascending, |2 sat - T| descending, phase ascending, mask ascending; the first `top`
    (None: all).  Per check a dict: phase, mask, extent, mask0 (the mask shifted down to its
    lowest symbol), template (of mask0 at span extent - 1: parity.py's (output, delay)
    terms), sat, T, z = (2 sat - T) / sqrt(T), inverted (z < 0: an odd-weight check on a
    polarity-inverted stream).

    For n = 3 a one-bit phase shift can keep a check's extent (seen on r23_m4): the list
    ranks the checks there but its first phase is not a claim about the symbol boundary."""
    n, max_span = int(n), int(max_span)
    B = _bits(n, max_span)
    dev = _device(device)
    cap, _, nbits = capture_buffer(capture, format, nbits, dev)
    if T is None:
        T = anchors_in(nbits, n, max_span, start, n)
    T = int(T)
    sat = parity_sweep(cap, n, max_span, start, T, n, format, nbits, dev)
    if T == 0:
        return []
    z_min = default_z_min(n, B) if z_min is None else float(z_min)
    d = 2 * sat - T
    keep = d.double() ** 2 >= z_min * z_min * T
    keep[:, 0] = False
    idx = torch.nonzero(keep)                       # filtered on the device, ranked on the host
    phases, masks = idx[:, 0].cpu().tolist(), idx[:, 1].cpu().tolist()
    sats = sat[keep].cpu().tolist()                 # row-major, the order of nonzero
    found = sorted(zip(phases, masks, sats),
                   key=lambda c: (mask_extent(c[1], n), -abs(2 * c[2] - T), c[0], c[1]))
    out = []
    for f, mask, s in found[:top]:
        extent = mask_extent(mask, n)
        mask0 = mask >> (n * (((mask & -mask).bit_length() - 1) // n))
        z = (2 * s - T) / math.sqrt(T)
        out.append({"phase": f, "mask": mask, "extent": extent, "mask0": mask0,
                    "template": mask_template(mask0, n, extent - 1), "sat": s, "T": T, "z": z,
                    "inverted": z < 0})
    return out


def identify_code(capture, max_span, start=0, T=None, format="bytes", nbits=None, z_min=None, device=None):
    """The k = 1, n = 2 code of a capture: the first-ranked check h = (h_0, h_1) of
    find_parity_checks is the shortest one, h_0 g_0 + h_1 g_1 = 0 with g_0 = h_1 and
    g_1 = h_0.  Returns {"m": extent - 1, "gen": [[h_1 taps]], [[h_0 taps]] (the package's
    gen[j][i][d], delay-ordered), "phase": the symbol phase of the check, "check": its
    find_parity_checks entry}, or None when no mask is significant.  (n = 3: see
    find_parity_checks; a k = 2 code has no such one-check reading.)"""
    checks = find_parity_checks(capture, 2, max_span, start, T, format, nbits, z_min, 1, device)
    if not checks:
        return None
    c = checks[0]
    m = c["extent"] - 1
    h = [[0] * (m + 1) for _ in range(2)]
    for j, s in c["template"]:
        h[j][s] = 1
    return {"m": m, "gen": [[h[1]], [h[0]]], "phase": c["phase"], "check": c}

"""Punctured soft frames (cvd_viterbi_decode_frames_soft_punctured and its tail-biting and
soft-output siblings, include/cvd.h) in numpy, for the host and the GPU tests: the per-frame
depuncture written from the header's text (v'_f), the puncturing that undoes it, builders of
captures of punctured soft frames, and what the terminated call's records [4], [5] are by the
header (a re-encoding of the decoded bits).  Nothing here knows the kernels."""
import numpy as np

import llr_cases as LC

# keep[c], bit j = output j of a step in column c is sent.  The DVB-S names are the library's
# PUNCTURE_PATTERNS (rows X / Y of oct:171,133); the host test checks that they agree.
PATTERNS = {
    "all2": (2, [3]),                                  # period 1, everything kept
    "dvb:2/3": (2, [3, 2]),                            # 10/11
    "dvb:3/4": (2, [3, 2, 1]),                         # 101/110
    "dvb:7/8": (2, [3, 2, 2, 2, 1, 2, 1]),             # 1000101/1111010
    "p16": (2, [3, 1, 2, 3, 2, 2, 1, 1, 3, 2, 1, 2, 1, 3, 1, 2]),
    "all3": (3, [7]),
    "n3": (3, [7, 4, 5, 3]),                           # a column with output 2 alone, one with 0 and 2: rank != j
}


def kept(keep):
    """The kept outputs per column."""
    return [bin(int(k)).count("1") for k in keep]


def pos(t, keep):
    """pos(t) - start: the values that steps 0..t-1 consume."""
    cnt = kept(keep)
    return (t // len(cnt)) * sum(cnt) + sum(cnt[:t % len(cnt)])


def depuncture_frame(vals, keep, n, T):
    """v'[n t + j] = vals[pos(t) + rank of j among the kept outputs of keep[t mod period]] where the
    column keeps j, and 0 otherwise; vals: the frame's pos(T) values."""
    out = np.zeros(n * T, dtype=np.int8)
    for t in range(T):
        k, p, rank = keep[t % len(keep)], pos(t, keep), 0
        for j in range(n):
            if (k >> j) & 1:
                out[n * t + j] = vals[p + rank]
                rank += 1
    assert T == 0 or p + rank == pos(T, keep) == len(vals)
    return out


def puncture_frame(v, keep, n, T):
    """The kept values of the n T values v, in order."""
    mask = np.array([(keep[t % len(keep)] >> j) & 1 for t in range(T) for j in range(n)], dtype=bool)
    return np.asarray(v)[mask]


def punctured_frame(rng, gen, n, m, keep, T, start_state, end_state, kind):
    """One frame as llr_cases.soft_frame makes it (kind: noisy, m128, pm1, zero; an encoded word in
    noise with erasures, the special values among the kept ones too), punctured."""
    v, _ = LC.soft_frame(rng, gen, n, m, T, start_state, end_state, kind)
    return puncture_frame(v, keep, n, T)


def tailbiting_frame(rng, gen, n, m, keep, T, sigma):
    """A tail-biting frame (the encoder starts in the state of its own last m bits) at amplitude 24
    in Gaussian noise of sigma * 24, punctured."""
    info = rng.integers(0, 2, T)
    s = 0
    for u in info[-m:] if T >= m else np.tile(info, m)[-m:]:
        s = ((s << 1) | int(u)) & ((1 << m) - 1)
    bits, end = LC.encode(gen, n, m, info, s)
    assert end == s
    x = (2.0 * bits - 1.0) * 24 + rng.normal(0.0, sigma * 24, n * T)
    return puncture_frame(np.clip(np.rint(x), -127, 127).astype(np.int8), keep, n, T)


def place(frames, offsets, nvals, rng):
    """A capture of nvals values, random where no frame lies, with frames[i] at offsets[i] (later
    frames over earlier ones; an offset whose frame does not fit is left out)."""
    cap = rng.integers(-60, 61, nvals).astype(np.int8)
    for fr, o in zip(frames, offsets):
        if 0 <= o and o + len(fr) <= nvals:
            cap[o:o + len(fr)] = fr
    return cap


def depunctured_capture(cap, keep, n, T, offsets):
    """The capture of the frames v'_f one after the other, n T values each, and their offsets in it
    (-1 for a frame that the punctured call skips: o < 0 or o + pos(T) > len(cap))."""
    span = pos(T, keep)
    out = np.zeros(n * T * len(offsets), dtype=np.int8)
    off = np.full(len(offsets), -1, dtype=np.int64)
    for f, o in enumerate(offsets):
        o = int(o)
        if 0 <= o and o + span <= len(cap):
            out[n * T * f:n * T * (f + 1)] = depuncture_frame(cap[o:o + span], keep, n, T)
            off[f] = n * T * f
    return out, off


def viterbi(gen, n, m, v, T, start_state, end_state):
    """The frames contract's decoder over the states at once: (distance, u [T], s_T, s_0).  Ties
    keep b = 0; s_T is end_state or the lowest-index state of minimal D_T."""
    S = 1 << m
    out = LC.branch_outputs(gen, n, m)
    cost = LC.step_costs(v, n, T)
    s = np.arange(S)
    u, p0 = s & 1, s >> 1
    p1 = p0 | (1 << (m - 1))
    o0, o1 = out[p0, u], out[p1, u]
    D = LC.boundary(start_state, S)
    dec = np.zeros((T, S), dtype=np.uint8)
    for t in range(T):
        c0, c1 = D[p0] + cost[t][o0], D[p1] + cost[t][o1]
        dec[t] = c1 < c0
        D = np.minimum(np.minimum(c0, c1), LC.INF)
    sT = int(end_state) if end_state is not None else int(np.argmin(D))
    bits = np.zeros(T, dtype=np.uint8)
    st = sT
    for t in range(T - 1, -1, -1):
        bits[t] = st & 1
        st = (st >> 1) | (int(dec[t][st]) << (m - 1))
    return int(D[sT]), bits, sT, st


def sign_count(gen, n, m, v, T, bits, s0):
    """(errors, counted) of a decoded frame: the values of v that are not 0, and those among them
    whose sign disagrees with the re-encoding of `bits` from s0."""
    enc, _ = LC.encode(gen, n, m, bits, s0)
    v = np.asarray(v, dtype=np.int64)
    seen = v != 0
    return int((seen & ((v > 0) != (enc == 1))).sum()), int(seen.sum())


def reference_frames(gen, n, m, cap, keep, T, offsets, start_state, end_state, check=None):
    """Every output of the terminated call: bits uint8 [F, 4w], frames int32 [F, 6], stats [6].
    check(v, dist, u, sT): called per decoded frame with the depunctured values."""
    F, w, span = len(offsets), (T + 31) // 32, pos(T, keep)
    rows = np.zeros((F, 32 * w), dtype=np.uint8)
    frames = np.zeros((F, 6), dtype=np.int32)
    for f, o in enumerate(offsets):
        o = int(o)
        if o < 0 or o + span > len(cap):
            frames[f] = [0, -1, -1, 1, 0, 0]
            continue
        v = depuncture_frame(cap[o:o + span], keep, n, T)
        dist, u, sT, s0 = viterbi(gen, n, m, v, T, start_state, end_state)
        if check is not None:
            check(v, dist, u, sT)
        err, cnt = sign_count(gen, n, m, v, T, u, s0)
        rows[f, :T] = u
        frames[f] = [dist, s0, sT, 0, err, cnt]
    bits = np.packbits(rows.reshape(F, 4 * w, 8), axis=2, bitorder="little").reshape(F, 4 * w)
    ok = frames[:, 3] == 0
    stats = [int(frames[ok, 0].sum()), int(ok.sum()), int((~ok).sum()), int(frames[ok, 4].sum()),
             int(frames[ok, 5].sum()), w]
    return bits, frames, stats

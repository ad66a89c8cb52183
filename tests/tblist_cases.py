"""cvd_viterbi_decode_frames_tailbiting_list's references and cases: the sequential decoder written
from the text of include/cvd.h twice (list by list in plain Python, and with the states of a step
side by side for the shapes of the GPU tests), the batch reference (rows, path records, frame
records, totals, skipped frames), and a circular encoder with a builder of tail-biting frames that
end in a CRC.  The generators, branch outputs and step costs are llr_cases.py's, the row packing
and the CRC list_cases.py's.  numpy only."""
import functools

import numpy as np

import list_cases as LS
import llr_cases as LC

DEFAULT_LAPS = 4
MAX_LAPS = 8
SKIPPED = [0, 1, 0, 0]


def _stop(closes, lap, laps, En, E):
    """Is lap `lap` the last: e* in B, or l = I, or l >= 2 and E^l = E^{l-1}."""
    return closes or lap == laps or (lap >= 2 and list(En) == list(E))


def tblist_frame_plain(gen, n, m, v, T, L, laps=DEFAULT_LAPS):
    """One frame by the header's rule, list by list in plain Python.  Returns (paths, status, laps
    run, |C|, repeated): paths is a list of (c, u uint8 [T], s_0, s_T) in order, repeated says that
    the last lap was the last because E repeated (and for no other reason)."""
    S = 1 << m
    out = LC.branch_outputs(gen, n, m)
    cost = LC.step_costs(v, n, T)
    E = [0] * S
    lap = 0
    while True:
        lap += 1
        A = [[E[s]] for s in range(S)]
        dec = []
        for t in range(T):
            nA, nd = [], []
            for s in range(S):
                u = s & 1
                cand = []
                for b in (0, 1):
                    ps = (s >> 1) | (b << (m - 1))
                    c = int(cost[t][out[ps, u]])
                    cand += [(a + c, b, r) for r, a in enumerate(A[ps])]
                cand.sort()
                cand = cand[:L]
                nA.append([c for c, _, _ in cand])
                nd.append([(b, r) for _, b, r in cand])
            A = nA
            dec.append(nd)
        D = [A[s][0] for s in range(S)]
        mn = min(D)
        es = D.index(mn)                                      # the lowest index
        a = {}
        for e in range(S):
            for r0 in range(len(A[e])):
                s, r = e, r0
                for t in range(T - 1, -1, -1):
                    b, r = dec[t][s][r]
                    s = (s >> 1) | (b << (m - 1))
                a[(e, r0)] = s
        closes = a[(es, 0)] == es
        En = [d - mn for d in D]
        if _stop(closes, lap, laps, En, E):
            repeated = not closes and lap < laps
            break
        E = En
    C = sorted((A[e][r] - E[s], e, r) for (e, r), s in a.items() if s == e)
    B = [e for e in range(S) if a[(e, 0)] == e]
    if closes:
        status, e0 = 0, es
    elif B:
        status, e0 = 2, min(B, key=lambda e: (D[e] - E[e], e))
    else:
        status, e0 = 3, es
    entries = [(D[e0] - E[a[(e0, 0)]], e0, 0)] + [x for x in C if (x[1], x[2]) != (e0, 0)][:L - 1]
    paths = []
    for c, sT, rT in entries:
        u = np.zeros(T, dtype=np.uint8)
        s, r = sT, rT
        for t in range(T - 1, -1, -1):
            u[t] = s & 1
            b, r = dec[t][s][r]
            s = (s >> 1) | (b << (m - 1))
        paths.append((c, u, s, sT))
    return paths, status, lap, len(C), repeated


def tblist_frame(gen, n, m, v, T, L, laps=DEFAULT_LAPS):
    """tblist_frame_plain with the states of a step side by side, as list_cases.list_frame: a list
    is a row of L values with ABSENT behind the present ones, and the order of the triple (c, b, r)
    is the order of the integer 16 c + 8 b + r.  Same result."""
    S = 1 << m
    ABSENT = LC.INF
    out = LC.branch_outputs(gen, n, m)
    cost = LC.step_costs(v, n, T)
    sp = np.arange(S)
    u_of = sp & 1
    ps = [sp >> 1, (sp >> 1) | (1 << (m - 1))]
    bc = [[cost[t][out[ps[b], u_of]][:, None] for b in (0, 1)] for t in range(T)]        # the branches' costs by step
    tag = np.concatenate([8 * b + np.arange(L) for b in (0, 1)])[None, :]
    E = np.zeros(S, dtype=np.int64)
    lap = 0
    while True:
        lap += 1
        A = np.full((S, L), ABSENT, dtype=np.int64)
        A[:, 0] = E
        dec = np.zeros((T, S, L), dtype=np.int64)                 # the column b L + r that took the rank
        for t in range(T):
            cand = np.concatenate([np.where(A[ps[b]] >= ABSENT, ABSENT, A[ps[b]] + bc[t][b]) for b in (0, 1)], axis=1)
            order = np.argsort(16 * cand + tag, axis=1, kind="stable")[:, :L]
            A = np.take_along_axis(cand, order, axis=1)
            dec[t] = order
        D = A[:, 0]
        mn = int(D.min())
        es = int(np.argmin(D))                                    # the lowest index
        s = np.repeat(sp[:, None], L, axis=1)                     # every entry's chain
        r = np.repeat(np.arange(L)[None, :], S, axis=0)
        for t in range(T - 1, -1, -1):
            col = dec[t, s, r]
            r = col % L
            s = (s >> 1) | ((col // L) << (m - 1))
        a = s
        closes = a[es, 0] == es
        En = D - mn
        if _stop(closes, lap, laps, En, E):
            repeated = not closes and lap < laps
            break
        E = En
    inC = (A < ABSENT) & (a == sp[:, None])
    C = sorted((int(A[e, q] - E[a[e, q]]), int(e), int(q)) for e, q in np.argwhere(inC))
    B = np.flatnonzero(inC[:, 0])
    if closes:
        status, e0 = 0, es
    elif len(B):
        status, e0 = 2, int(min(B, key=lambda e: (D[e] - E[e], e)))
    else:
        status, e0 = 3, es
    entries = [(int(D[e0] - E[a[e0, 0]]), e0, 0)] + [x for x in C if (x[1], x[2]) != (e0, 0)][:L - 1]
    paths = []
    for c, sT, rT in entries:
        u = np.zeros(T, dtype=np.uint8)
        s, r = sT, rT
        for t in range(T - 1, -1, -1):
            u[t] = s & 1
            col = int(dec[t, s, r])
            r = col % L
            s = (s >> 1) | ((col // L) << (m - 1))
        paths.append((c, u, s, sT))
    return paths, status, lap, len(C), repeated


def reference_batch(gen, n, m, soft, T, L, offsets, laps=DEFAULT_LAPS):
    """Every output of the call for frames at `offsets` (those outside [0, len(soft)) skipped):
    bits uint8 [F, L, 4w], paths int32 [F, L, 3], frames int32 [F, 4], stats [8], and which frames
    stopped because E repeated (bool [F])."""
    F, w = len(offsets), (T + 31) // 32
    rows = np.zeros((F, L, 32 * w), dtype=np.uint8)
    paths = np.full((F, L, 3), -1, dtype=np.int32)
    frames = np.zeros((F, 4), dtype=np.int32)
    repeated = np.zeros(F, dtype=bool)
    dist0 = 0
    for f, o in enumerate(offsets):
        o = int(o)
        if o < 0 or o + n * T > len(soft):
            frames[f] = SKIPPED
            continue
        found, status, lap, nC, repeated[f] = tblist_frame(gen, n, m, soft[o:o + n * T], T, L, laps)
        for l, (c, u, s0, sT) in enumerate(found):
            rows[f, l, :T] = u
            paths[f, l] = [c, s0, sT]
        frames[f] = [len(found), status, lap, nC]
        dist0 += found[0][0]
    ok = frames[:, 1] != 1
    stats = [dist0, int(ok.sum()), int((~ok).sum()), int(frames[:, 0].sum()), w, int((frames[:, 1] == 2).sum()),
             int((frames[:, 1] == 3).sum()), int(frames[:, 2].sum())]
    return LS.pack_rows(rows, w), paths, frames, stats, repeated


def encode_circular(gen, n, m, u):
    """The n T output bits of the tail-biting frame u: the encoder starts in the state that the
    frame's own last m bits leave it in (bit d - 1 of the state = u[(T - d) mod T]), and ends there."""
    T = len(u)
    state = 0
    for d in range(1, m + 1):
        state |= int(u[(T - d) % T]) << (d - 1)
    bits, end = LC.encode(gen, n, m, u, state)
    assert end == state
    return bits, state


def noisy(rng, coded, amplitude, sigma):
    """The int8 values of the bits `coded` at +-amplitude in Gaussian noise of sigma * amplitude."""
    x = (2.0 * coded - 1.0) * amplitude + rng.normal(0.0, sigma * amplitude, len(coded))
    return np.clip(np.rint(x), -127, 127).astype(np.int8)


def tailbiting_frames(rng, gen, n, m, F, T, amplitude=24, sigma=1.3):
    """F tail-biting frames of random bits one after the other: (soft int8 [F n T], sent uint8 [F, T])."""
    sent = rng.integers(0, 2, (F, T)).astype(np.uint8)
    soft = np.concatenate([noisy(rng, encode_circular(gen, n, m, sent[f])[0], amplitude, sigma) for f in range(F)])
    return soft, sent


def crc_frames(rng, gen, n, m, F, data_bits, crc, amplitude, sigma, mask=0):
    """F tail-biting frames of data || CRC ^ mask (an LTE PBCH or DCI: no tail), as int8 values in
    Gaussian noise: (soft int8 [F n T], sent uint8 [F, T], T)."""
    width, poly, init, expect = LS.CRC_SPECS[crc]
    T = data_bits + width
    sent = np.zeros((F, T), dtype=np.uint8)
    soft = np.zeros((F, n * T), dtype=np.int8)
    for f in range(F):
        data = rng.integers(0, 2, data_bits).astype(np.uint8)
        sent[f] = LS.crc_append(data, width, poly, init, expect ^ mask)
        soft[f] = noisy(rng, encode_circular(gen, n, m, sent[f])[0], amplitude, sigma)
    return soft.reshape(-1), sent, T


# The inputs of the GPU tests that must cover every outcome of the rule (tests/test_decode_tblist_host.py
# asserts the counts on the reference): (m, n, T, F, sigma, seed)
COVERING = [(6, 3, 40, 300, 1.5, 1), (6, 2, 24, 300, 1.4, 2), (3, 2, 12, 300, 1.3, 3)]


@functools.lru_cache(maxsize=None)
def covering_capture(m, n, T, F, sigma, seed):
    gen = LC.gen_of(m, n)
    soft, _ = tailbiting_frames(np.random.default_rng(seed), gen, n, m, F, T, 24, sigma)
    soft.setflags(write=False)
    return gen, soft


@functools.lru_cache(maxsize=None)
def covering_reference(i, L, laps=DEFAULT_LAPS):
    """reference_batch of COVERING[i], the frames one after the other (computed once, not written to)."""
    m, n, T, F, sigma, seed = COVERING[i]
    gen, soft = covering_capture(m, n, T, F, sigma, seed)
    ref = reference_batch(gen, n, m, soft, T, L, n * T * np.arange(F), laps)
    for a in ref[:3] + ref[4:]:
        a.setflags(write=False)
    return ref

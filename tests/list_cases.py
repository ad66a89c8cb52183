"""cvd_viterbi_decode_frames_list's and cvd_frames_crc's references and cases: the sequential list
decoder written from the text of include/cvd.h (lists of at most L values per state, the order
(c, b, r), the end list, the traceback through (state, rank)), the batch reference (rows, path
records, frame records, totals, skipped frames), and the bit-serial CRC with its field.  The
generators, branch outputs, step costs, frame builder and the independent Viterbi decoder are
llr_cases.py's.  numpy only."""
import numpy as np

import llr_cases as LC

MAX_L = 8
MAX_T = 8192

CRC_SPECS = {            # name: (width, poly, init, expect)
    "crc8-lte": (8, 0x9B, 0, 0),
    "crc16-ccitt": (16, 0x1021, 0, 0),
    "crc24a": (24, 0x864CFB, 0, 0),
    "crc24b": (24, 0x800063, 0, 0),
    "crc32": (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF),
}


def list_frame_plain(gen, n, m, v, T, L, start_state=0, end_state=0):
    """One frame by the header's recursion, list by list in plain Python.  Returns the paths found,
    in order: a list of (distance, u uint8 [T], s_0, s_T)."""
    S = 1 << m
    out = LC.branch_outputs(gen, n, m)
    cost = LC.step_costs(v, n, T)
    A = [[0] if start_state is None or s == start_state else [] for s in range(S)]
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
    if end_state is not None:
        ends = [(a, end_state, r) for r, a in enumerate(A[end_state])]
    else:
        ends = sorted((a, s, r) for s in range(S) for r, a in enumerate(A[s]))[:L]
    paths = []
    for dist, sT, rT in ends:
        u = np.zeros(T, dtype=np.uint8)
        s, r = sT, rT
        for t in range(T - 1, -1, -1):
            u[t] = s & 1
            b, r = dec[t][s][r]
            s = (s >> 1) | (b << (m - 1))
        paths.append((dist, u, s, sT))
    return paths


def list_frame(gen, n, m, v, T, L, start_state=0, end_state=0):
    """list_frame_plain with the states of a step side by side (the large shapes of the GPU tests
    need it): a list is a row of L values with ABSENT behind the present ones, and the order of the
    triple (c, b, r) is the order of the integer 16 c + 8 b + r (r < 8).  Same result."""
    S = 1 << m
    ABSENT = LC.INF
    out = LC.branch_outputs(gen, n, m)
    cost = LC.step_costs(v, n, T)
    sp = np.arange(S)
    u_of = sp & 1
    ps = [sp >> 1, (sp >> 1) | (1 << (m - 1))]
    tag = np.concatenate([8 * b + np.arange(L) for b in (0, 1)])[None, :]         # 8 b + r of candidate column b L + r
    A = np.full((S, L), ABSENT, dtype=np.int64)
    if start_state is None:
        A[:, 0] = 0
    else:
        A[start_state, 0] = 0
    dec = np.zeros((T, S, L), dtype=np.uint8)                                     # the column b L + r that took the rank
    for t in range(T):
        cand = np.concatenate([np.where(A[ps[b]] >= ABSENT, ABSENT, A[ps[b]] + cost[t][out[ps[b], u_of]][:, None])
                               for b in (0, 1)], axis=1)
        order = np.argsort(16 * cand + tag, axis=1, kind="stable")[:, :L]
        A = np.take_along_axis(cand, order, axis=1)
        dec[t] = order
    if end_state is not None:
        ends = [(int(a), end_state, r) for r, a in enumerate(A[end_state]) if a < ABSENT]
    else:
        ends = sorted((int(A[s, r]), s, r) for s in range(S) for r in range(L) if A[s, r] < ABSENT)[:L]
    paths = []
    for dist, sT, rT in ends:
        u = np.zeros(T, dtype=np.uint8)
        s, r = sT, rT
        for t in range(T - 1, -1, -1):
            u[t] = s & 1
            col = int(dec[t, s, r])
            b, r = col // L, col % L
            s = (s >> 1) | (b << (m - 1))
        paths.append((dist, u, s, sT))
    return paths


def pack_rows(rows, w):
    """uint8 [..., 32 w] of bits -> uint8 [..., 4 w], LSB first."""
    return np.packbits(rows.reshape(rows.shape[:-1] + (4 * w, 8)), axis=-1, bitorder="little").reshape(
        rows.shape[:-1] + (4 * w,))


def unpack_rows(bits):
    """uint8 [..., 4 w] -> uint8 [..., 32 w] of bits, LSB first."""
    return np.unpackbits(np.ascontiguousarray(bits), axis=-1, bitorder="little")


def reference_batch(gen, n, m, soft, T, L, offsets, start_state, end_state):
    """Every output of the call for frames at `offsets` (those outside [0, len(soft)) skipped):
    bits uint8 [F, L, 4w], paths int32 [F, L, 3], frames int32 [F, 2], stats [5]."""
    F, w = len(offsets), (T + 31) // 32
    rows = np.zeros((F, L, 32 * w), dtype=np.uint8)
    paths = np.full((F, L, 3), -1, dtype=np.int32)
    frames = np.zeros((F, 2), dtype=np.int32)
    dist0 = 0
    for f, o in enumerate(offsets):
        o = int(o)
        if o < 0 or o + n * T > len(soft):
            frames[f] = [0, 1]
            continue
        found = list_frame(gen, n, m, soft[o:o + n * T], T, L, start_state, end_state)
        for l, (dist, u, s0, sT) in enumerate(found):
            rows[f, l, :T] = u
            paths[f, l] = [dist, s0, sT]
        frames[f] = [len(found), 0]
        dist0 += found[0][0]
    ok = frames[:, 1] == 0
    stats = [dist0, int(ok.sum()), int((~ok).sum()), int(frames[:, 0].sum()), w]
    return pack_rows(rows, w), paths, frames, stats


def crc_bits(u, width, poly, init=0):
    """The register after the bits u, by the header's loop."""
    mask = (1 << width) - 1
    reg = init & mask
    for b in u:
        fb = ((reg >> (width - 1)) & 1) ^ int(b)
        reg = (reg << 1) & mask
        if fb:
            reg ^= poly
    return reg


def crc_value(u, first, count, width, poly, init=0):
    """d_value of one row of bits u (a sequence of 0 / 1): reg ^ field."""
    reg = crc_bits(u[first:first + count], width, poly, init)
    field = 0
    for i in range(width):
        field |= int(u[first + count + i]) << (width - 1 - i)
    return reg ^ field


def crc_append(data, width, poly, init=0, xor=0):
    """data followed by the width bits of its CRC ^ xor, first bit most significant."""
    reg = crc_bits(data, width, poly, init) ^ xor
    return np.concatenate([np.asarray(data, dtype=np.uint8),
                           np.array([(reg >> (width - 1 - i)) & 1 for i in range(width)], dtype=np.uint8)])


def reference_crc(bits, first, count, width, poly, init=0):
    """crc_value of every row of packed bits uint8 [..., 4w]: int64 of the leading shape."""
    u = unpack_rows(bits)
    flat = u.reshape(-1, u.shape[-1])
    vals = np.array([crc_value(r, first, count, width, poly, init) for r in flat], dtype=np.int64)
    return vals.reshape(u.shape[:-1])


def select(values, present, expect):
    """choice int32 [F]: the lowest present l with values[f, l] == expect, -1 if none."""
    hit = (np.asarray(values) == expect) & np.asarray(present)
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int32)


def crc_frames(rng, gen, n, m, F, data_bits, crc, amplitude, sigma):
    """F terminated frames of data || CRC || m zero tail bits from state 0, as int8 values in
    Gaussian noise: (soft int8 [F n T], sent uint8 [F, T], T)."""
    width, poly, init, expect = CRC_SPECS[crc]
    T = data_bits + width + m
    sent = np.zeros((F, T), dtype=np.uint8)
    soft = np.zeros((F, n * T), dtype=np.int8)
    for f in range(F):
        data = rng.integers(0, 2, data_bits).astype(np.uint8)
        sent[f, :data_bits + width] = crc_append(data, width, poly, init, expect)
        coded, _ = LC.encode(gen, n, m, sent[f], 0)
        x = (2.0 * coded - 1.0) * amplitude + rng.normal(0.0, sigma * amplitude, n * T)
        soft[f] = np.clip(np.rint(x), -127, 127).astype(np.int8)
    return soft.reshape(-1), sent, T

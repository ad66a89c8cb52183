"""cvd_viterbi_decode_frames_llr's reference and cases: the sequential decoder written from the text
of include/cvd.h (alpha, beta, M_u, the saturation rule, the record of a frame, the totals), an
independent Viterbi decoder with traceback for the contract's identities, and the builders of the
soft frames that the host and the GPU tests share.  numpy only."""
import numpy as np

INF = 1 << 40            # +inf: above every finite metric, and sums of two stay exact in int64
SAT = 32767

GENS = {                 # k = 1 codes by (m, n): the generators' octal digits
    (1, 2): (3, 1), (2, 2): (7, 5), (3, 2): (15, 17), (4, 2): (23, 35), (5, 2): (53, 75), (6, 2): (133, 171),
    (7, 2): (247, 371), (8, 2): (561, 753), (6, 3): (133, 171, 165), (8, 3): (557, 663, 711),
}


def gen_of(m, n):
    """gen[j][0][d] of GENS[(m, n)]: the octal's MSB is the tap of the current input (delay 0)."""
    return [[[(int(str(g), 8) >> (m - d)) & 1 for d in range(m + 1)]] for g in GENS[(m, n)]]


def is_inf(x):
    return x >= INF // 2


def branch_outputs(gen, n, m):
    """out[s, u]: the n output bits (bit j = output j) of the branch from state s with input u;
    bit d - 1 of s is the input of d steps ago."""
    S = 1 << m
    out = np.zeros((S, 2), dtype=np.int64)
    for s in range(S):
        for u in (0, 1):
            o = 0
            for j in range(n):
                b = gen[j][0][0] & u
                for d in range(1, m + 1):
                    b ^= gen[j][0][d] & (s >> (d - 1)) & 1
                o |= b << j
            out[s, u] = o
    return out


def step_costs(v, n, T):
    """cost[t, o] = sum_j a(v_tj) [v_tj != 0 and (v_tj > 0) != bit j of o], -128 read as -127."""
    v = np.maximum(np.asarray(v, dtype=np.int64).reshape(T, n), -127)
    cost = np.zeros((T, 1 << n), dtype=np.int64)
    for o in range(1 << n):
        for j in range(n):
            bit = (o >> j) & 1
            cost[:, o] += np.abs(v[:, j]) * ((v[:, j] != 0) & ((v[:, j] > 0) != bool(bit)))
    return cost


def boundary(state, S):
    if state is None:
        return np.zeros(S, dtype=np.int64)
    x = np.full(S, INF, dtype=np.int64)
    x[state] = 0
    return x


def reference_frame(gen, n, m, v, T, start_state=0, end_state=0):
    """One frame by the header's recursion.  Returns a dict: llr (int64 [T]), bits (uint8 [T]),
    record (the six fields), M0, M1 (int64 [T], INF-class values where infinite)."""
    S = 1 << m
    out = branch_outputs(gen, n, m)
    cost = step_costs(v, n, T)
    sp = np.arange(S)
    u_of = sp & 1
    ps = [sp >> 1, (sp >> 1) | (1 << (m - 1))]
    ns = [((sp << 1) | u) & (S - 1) for u in (0, 1)]
    alpha = np.empty((T + 1, S), dtype=np.int64)
    alpha[0] = boundary(start_state, S)
    for t in range(T):
        c0 = alpha[t][ps[0]] + cost[t][out[ps[0], u_of]]
        c1 = alpha[t][ps[1]] + cost[t][out[ps[1], u_of]]
        alpha[t + 1] = np.minimum(np.minimum(c0, c1), INF)
    beta = np.empty((T + 1, S), dtype=np.int64)
    beta[T] = boundary(end_state, S)
    for t in range(T - 1, -1, -1):
        b0 = cost[t][out[sp, 0]] + beta[t + 1][ns[0]]
        b1 = cost[t][out[sp, 1]] + beta[t + 1][ns[1]]
        beta[t] = np.minimum(np.minimum(b0, b1), INF)
    tot = np.minimum(alpha[1:] + beta[1:], INF)                # [T, S]
    M0 = tot[:, 0::2].min(axis=1)
    M1 = tot[:, 1::2].min(axis=1)
    assert not (is_inf(M0) & is_inf(M1)).any()
    llr = np.where(is_inf(M0), SAT, np.where(is_inf(M1), -SAT, M0 - M1))
    sat = np.abs(llr) == SAT
    dist = np.minimum(M0, M1)
    assert (dist == dist[0]).all()
    sT = end_state if end_state is not None else int(np.argmin(alpha[T]))     # the lowest index of the minimum
    weakest = int(np.abs(llr[~sat]).min()) if (~sat).any() else SAT
    record = [int(dist[0]), int((llr == 0).sum()), int(sT), 0, weakest, int(sat.sum())]
    return {"llr": llr, "bits": (llr > 0).astype(np.uint8), "record": record, "M0": M0, "M1": M1}


def viterbi_frame(gen, n, m, v, T, start_state=0, end_state=0):
    """The frames contract's decoder, written independently of reference_frame: forward pass with
    the tie rule (`val < best`, ties keep b = 0), the end-state rule, traceback.  Returns
    (distance, u [T], s_T)."""
    S = 1 << m
    out = branch_outputs(gen, n, m)
    cost = step_costs(v, n, T)
    D = [0 if start_state is None or s == start_state else INF for s in range(S)]
    dec = []
    for t in range(T):
        nd, dd = [0] * S, [0] * S
        for s in range(S):
            u, p0 = s & 1, s >> 1
            p1 = p0 | (1 << (m - 1))
            c0, c1 = D[p0] + int(cost[t][out[p0, u]]), D[p1] + int(cost[t][out[p1, u]])
            dd[s] = int(c1 < c0)
            nd[s] = min(min(c0, c1), INF)
        D = nd
        dec.append(dd)
    sT = end_state if end_state is not None else min(range(S), key=lambda s: (D[s], s))
    u = np.zeros(T, dtype=np.uint8)
    s = sT
    for t in range(T - 1, -1, -1):
        u[t] = s & 1
        s = (s >> 1) | (dec[t][s] << (m - 1))
    return D[sT], u, sT


def encode(gen, n, m, info, state):
    """The n T output bits of the info bits from `state`, and the state after them."""
    out = branch_outputs(gen, n, m)
    S = 1 << m
    bits = np.zeros(n * len(info), dtype=np.uint8)
    for t, u in enumerate(info):
        o = out[state, int(u)]
        for j in range(n):
            bits[n * t + j] = (o >> j) & 1
        state = ((state << 1) | int(u)) & (S - 1)
    return bits, state


def soft_frame(rng, gen, n, m, T, start_state, end_state, kind="noisy", amplitude=24, sigma=0.7):
    """The int8 values of one frame whose encoder starts in start_state (None: a random state) and,
    where T >= m, ends in end_state (None: wherever the random bits leave it).
    kind: "noisy" +-A in Gaussian noise with 3% erasures; "m128" the same with a tenth of the
    values replaced by -128; "zero" every value 0; "pm1" the signs at magnitude 1 under twice the
    noise, so that equal costs, and with them values of 0, are common."""
    if kind == "pm1":
        sigma = 2 * sigma
    S = 1 << m
    info = rng.integers(0, 2, T)
    if end_state is not None and T >= m:
        for i in range(m):
            info[T - 1 - i] = (end_state >> i) & 1
    s = int(rng.integers(0, S)) if start_state is None else start_state
    bits, _ = encode(gen, n, m, info, s)
    x = (2.0 * bits - 1.0) * amplitude + rng.normal(0.0, sigma * amplitude, n * T)
    v = np.clip(np.rint(x), -127, 127).astype(np.int8)
    v[rng.random(n * T) < 0.03] = 0
    if kind == "m128":
        v[rng.random(n * T) < 0.1] = -128
    elif kind == "zero":
        v[:] = 0
    elif kind == "pm1":
        v = np.sign(v).astype(np.int8)
    else:
        assert kind == "noisy", kind
    return v, info.astype(np.uint8)


def reference_batch(gen, n, m, soft, T, offsets, start_state, end_state):
    """Every output of the call for frames at `offsets` (those outside [0, len(soft)) skipped):
    llr int16 [F, T], bits uint8 [F, 4w] (LSB-packed rows), frames int32 [F, 6], stats [6]."""
    F, w = len(offsets), (T + 31) // 32
    llr = np.zeros((F, T), dtype=np.int16)
    rows = np.zeros((F, 32 * w), dtype=np.uint8)
    frames = np.zeros((F, 6), dtype=np.int32)
    for f, o in enumerate(offsets):
        o = int(o)
        if o < 0 or o + n * T > len(soft):
            frames[f] = [0, 0, -1, 1, 0, 0]
            continue
        r = reference_frame(gen, n, m, soft[o:o + n * T], T, start_state, end_state)
        llr[f] = r["llr"]
        rows[f, :T] = r["bits"]
        frames[f] = r["record"]
    bits = np.packbits(rows.reshape(F, 4 * w, 8), axis=2, bitorder="little").reshape(F, 4 * w)
    ok = frames[:, 3] == 0
    stats = [int(frames[ok, 0].sum()), int(ok.sum()), int((~ok).sum()), int(frames[ok, 1].sum()),
             int(frames[ok, 5].sum()), w]
    return llr, bits, frames, stats

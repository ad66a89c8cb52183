"""cvd_viterbi_decode_frames_tailbiting, _punctured and _soft on the GPU against a sequential
numpy decoder written from the contract in include/cvd.h (the wrap-around Viterbi algorithm:
laps from the normalised end vector of the lap before, all end states traced, the stopping rule
and the choice of the returned survivor): the rows of bits, all eight fields of every frame's
record and all nine totals are compared exactly.  The small helpers (trellis, costs, packing)
are restated from tests/test_gpu_decode_frames.py; the encoder here is circular."""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIG = 1 << 40
# k = 1 generators in octal, MSB = the current input
OCT = {(1, 2): (3, 1), (2, 2): (7, 5), (5, 2): (53, 75), (6, 2): (133, 171), (7, 2): (247, 371), (8, 2): (561, 753),
       (6, 3): (133, 171, 165), (8, 3): (557, 663, 711)}
SKIPPED = [0, -1, -1, 1, 0, 0, 0, 0]


def gen_of(m, n):
    return [[[(int(str(g), 8) >> (m - d)) & 1 for d in range(m + 1)]] for g in OCT[(m, n)]]


def trellis(n, m, gen):
    """ps[b][s'], out[b][s']: predecessor b of next state s' and the output word of that branch."""
    S = 1 << m
    s1 = np.arange(S)
    u = s1 & 1
    ps = np.stack([s1 >> 1, (s1 >> 1) | (1 << (m - 1))])
    out = np.zeros((2, S), dtype=np.int64)
    for j in range(n):
        bit = gen[j][0][0] * u
        bit = np.stack([bit, bit])
        for d in range(1, m + 1):
            bit = bit ^ (gen[j][0][d] * ((ps >> (d - 1)) & 1))
        out |= bit << j
    return ps, out


def encode_circular(n, m, gen, u):
    """Output words [F, T] of the tail-biting frames u [F, T]: u_{t-d} is taken mod T."""
    y = np.zeros(u.shape, dtype=np.int64)
    for j in range(n):
        bit = np.zeros(u.shape, dtype=np.int64)
        for d in range(m + 1):
            if gen[j][0][d]:
                bit ^= np.roll(u, d, axis=1)
        y |= bit << j
    return y


def wrap_state(m, u):
    """The state the encoder of a tail-biting frame starts and ends in: bit d - 1 = u_{T-d mod T}."""
    T = u.shape[1]
    return sum(u[:, (T - d) % T] << (d - 1) for d in range(1, m + 1))


def ref_tailbiting(n, m, gen, cost, laps):
    """The contract's decoder over cost[F, T, 2^n] (the metric of output word o at step t) with
    max_laps = laps: bits [F, T], rec [F, 8] (fields 4 and 5 left 0), the returned paths' output
    words [F, T], and which frames stopped before lap `laps` because E repeated."""
    F, T, _ = cost.shape
    S = 1 << m
    ps, out = trellis(n, m, gen)
    states = np.arange(S)
    E = np.zeros((F, S), dtype=np.int64)
    bits = np.zeros((F, T), dtype=np.uint8)
    words = np.zeros((F, T), dtype=np.int64)
    rec = np.zeros((F, 8), dtype=np.int64)
    repeated = np.zeros(F, dtype=bool)
    active = np.arange(F)
    for lap in range(1, laps + 1):
        c, D0 = cost[active], E[active]
        A = len(active)
        rows = np.arange(A)
        D = D0.copy()
        dec = np.zeros((A, T, S), dtype=bool)
        for t in range(T):
            c0 = D[:, ps[0]] + c[:, t][:, out[0]]
            c1 = D[:, ps[1]] + c[:, t][:, out[1]]
            dec[:, t] = c1 < c0                              # ties keep b = 0
            D = np.minimum(c0, c1)
        En = D - D.min(axis=1, keepdims=True)
        s = np.tile(states, (A, 1))                          # every end state's chain
        for t in range(T - 1, -1, -1):
            s = (s >> 1) | (dec[rows[:, None], t, s].astype(np.int64) << (m - 1))
        inB = s == states[None, :]
        cc = D - np.take_along_axis(D0, s, axis=1)
        es = np.argmin(D, axis=1)                            # argmin: the lowest index
        closes = inB[rows, es]
        same = (En == D0).all(axis=1) if lap >= 2 else np.zeros(A, dtype=bool)
        stop = closes | same | (lap == laps)
        anyB = inB.any(axis=1)
        eB = np.argmin(np.where(inB, cc, BIG), axis=1)
        e = np.where(closes | ~anyB, es, eB)
        status = np.where(closes, 0, np.where(anyB, 2, 3))
        repeated[active] = ~closes & same & (lap < laps)
        k = np.flatnonzero(stop)
        f = active[k]
        sc = e[k].copy()
        for t in range(T - 1, -1, -1):
            bits[f, t] = sc & 1
            b = dec[k, t, sc].astype(np.int64)
            words[f, t] = out[b, sc]
            sc = (sc >> 1) | (b << (m - 1))
        assert np.array_equal(sc, s[k, e[k]])
        rec[f, 0], rec[f, 1], rec[f, 2], rec[f, 3], rec[f, 6] = cc[k, e[k]], sc, e[k], status[k], lap
        E[active] = En
        active = active[~stop]
    assert len(active) == 0
    return bits, rec, words, repeated


def ref_any_any(n, m, gen, cost):
    """The bits [F, T] of decode_frames(start_state=None, end_state=None): one lap from the zero
    vector and the survivor of the lowest-index best end state, tail-biting or not."""
    F, T, _ = cost.shape
    ps, out = trellis(n, m, gen)
    D = np.zeros((F, 1 << m), dtype=np.int64)
    dec = np.zeros((F, T, 1 << m), dtype=bool)
    for t in range(T):
        c0 = D[:, ps[0]] + cost[:, t][:, out[0]]
        c1 = D[:, ps[1]] + cost[:, t][:, out[1]]
        dec[:, t] = c1 < c0
        D = np.minimum(c0, c1)
    s = np.argmin(D, axis=1)
    bits = np.zeros((F, T), dtype=np.uint8)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s & 1
        s = (s >> 1) | (dec[np.arange(F), t, s].astype(np.int64) << (m - 1))
    return bits


POP = np.array([bin(v).count("1") for v in range(8)], dtype=np.int64)


def hard_cost(n, y, keep=None):
    """cost[F, T, 2^n] of received words y [F, T]; keep [T]: the kept outputs of each step."""
    o = np.arange(1 << n)
    x = y[:, :, None] ^ o[None, None, :]
    if keep is not None:
        x = x & keep[None, :, None]
    return POP[x]


def soft_values(n, v):
    """a [F, T, n], nonzero [F, T, n], says-one [F, T, n] of the values v [F, T, n]."""
    v = v.astype(np.int64)
    return np.minimum(np.abs(v), 127), v != 0, v > 0


def soft_cost(n, v):
    a, nz, one = soft_values(n, v)
    cost = np.zeros(v.shape[:2] + (1 << n,), dtype=np.int64)
    for o in range(1 << n):
        for j in range(n):
            cost[:, :, o] += a[:, :, j] * (nz[:, :, j] & (one[:, :, j] != bool((o >> j) & 1)))
    return cost


def pack_rows(bits):
    """uint8 [F, 4 w] of bits [F, T], LSB first, zero padding."""
    F, T = bits.shape
    w = (T + 31) // 32
    pad = np.zeros((F, 32 * w), dtype=np.uint8)
    pad[:, :T] = bits
    return np.packbits(pad, axis=1, bitorder="little")


def frame_positions(n, T, keep=None):
    """pos[T][n] relative to a frame's start (-1: not transmitted), the keep mask per step, span."""
    pos = np.full((T, n), -1, dtype=np.int64)
    masks = np.zeros(T, dtype=np.int64)
    p = 0
    for t in range(T):
        kc = (1 << n) - 1 if keep is None else keep[t % len(keep)]
        masks[t] = kc
        for j in range(n):
            if (kc >> j) & 1:
                pos[t, j] = p
                p += 1
    return pos, masks, p


def received_words(capbits, offsets, pos):
    """y [F, T] of the frames at `offsets` in the bit array capbits (erased outputs read as 0)."""
    idx = offsets[:, None, None] + np.maximum(pos, 0)[None]
    b = capbits[idx].astype(np.int64) * (pos >= 0)[None]
    return (b << np.arange(pos.shape[1])[None, None, :]).sum(axis=2)


def as_capture(capbits, format):
    if format == "bytes":
        return capbits.copy()
    return np.packbits(capbits, bitorder="little" if format == "lsb" else "big")


def reference(n, m, gen, capbits, offsets, T, laps, keep=None, soft=None):
    """What decode_frames_tailbiting / _soft must return for frames at `offsets` (all inside the
    capture) with max_laps = laps: bits uint8 [F, 4w], frames int64 [F, 8], and the frames that
    stopped early because E repeated."""
    pos, masks, span = frame_positions(n, T, keep)
    if soft is None:
        y = received_words(capbits, offsets, pos)
        bits, rec, words, rep = ref_tailbiting(n, m, gen, hard_cost(n, y, None if keep is None else masks), laps)
        rec[:, 4], rec[:, 5] = rec[:, 0], span
    else:
        v = soft[offsets[:, None, None] + pos[None]]
        bits, rec, words, rep = ref_tailbiting(n, m, gen, soft_cost(n, v), laps)
        _, nz, one = soft_values(n, v)
        path = ((words[:, :, None] >> np.arange(n)[None, None, :]) & 1).astype(bool)
        rec[:, 4], rec[:, 5] = (nz & (one != path)).sum(axis=(1, 2)), nz.sum(axis=(1, 2))
    return pack_rows(bits), rec, rep


def check(res, want_bits, want_rec, T):
    """The GPU result against the reference's rows and records, and the totals against their sums."""
    got_bits, got_rec = res["bits"].cpu().numpy(), res["frames"].cpu().numpy().astype(np.int64)
    assert res["frames"].dtype == torch.int32 and got_rec.shape == want_rec.shape == (len(want_rec), 8)
    assert got_bits.dtype == np.uint8 and got_bits.shape == want_bits.shape
    assert np.array_equal(got_rec, want_rec), (np.argwhere(got_rec != want_rec)[:10], got_rec[:3], want_rec[:3])
    assert np.array_equal(got_bits, want_bits), np.argwhere(got_bits != want_bits)[:10]
    ok = want_rec[:, 3] != 1
    assert res["T"] == T and res["F"] == len(want_rec)
    totals = [res["total_distance"], res["decoded"], res["skipped"], res["total_errors"], res["total_counted"],
              res["words"], res["fallback"], res["open"], res["total_laps"]]
    assert totals == [int(want_rec[ok, 0].sum()), int(ok.sum()), int((~ok).sum()), int(want_rec[ok, 4].sum()),
                      int(want_rec[ok, 5].sum()), (T + 31) // 32, int((want_rec[:, 3] == 2).sum()),
                      int((want_rec[:, 3] == 3).sum()), int(want_rec[:, 6].sum())]
    for i, name in enumerate(["distance", "start_states", "end_states", "status", "errors", "counted", "laps"]):
        assert np.array_equal(res[name].cpu().numpy(), want_rec[:, i])
    assert res["ber"] == (res["total_errors"] / res["total_counted"] if res["total_counted"] else 0.0)


def tailbiting_capture(n, m, gen, T, F, stride, start, seed, p=0.05, keep=None):
    """A bit array holding F tail-biting frames of random data at start + f stride, sent through a
    BSC(p); the offsets and the data."""
    rng = np.random.default_rng(seed)
    pos, _, span = frame_positions(n, T, keep)
    u = rng.integers(0, 2, size=(F, T), dtype=np.int64)
    y = encode_circular(n, m, gen, u)
    nbits = start + (F - 1) * stride + span
    capbits = rng.integers(0, 2, size=nbits, dtype=np.uint8)
    flip = rng.random((F, T, n)) < p
    for f in range(F):                                   # in order: an overlapping frame overwrites its neighbour
        for j in range(n):
            sent = pos[:, j] >= 0
            capbits[start + f * stride + pos[sent, j]] = ((y[f, sent] >> j) & 1) ^ flip[f, sent, j]
    return capbits, start + stride * np.arange(F, dtype=np.int64), u


def run_case(pkg, m, n, T, F, stride_extra=0, format="bytes", laps=None, seed=1, p=0.05):
    gen = gen_of(m, n)
    stride = n * T + stride_extra
    capbits, offsets, _ = tailbiting_capture(n, m, gen, T, F, stride, 3, seed, p=p)
    res = pkg.decode_frames_tailbiting(n, m, gen, as_capture(capbits, format), T, F=F, start=3, stride=stride,
                                       max_laps=laps, format=format, nbits=len(capbits))
    want_bits, want_rec, _ = reference(n, m, gen, capbits, offsets, T, laps or 4)
    check(res, want_bits, want_rec, T)
    return res, want_rec


@pytest.mark.parametrize("m,n", sorted(OCT))
def test_code_shapes(pkg, m, n):
    """Fewer than 64 states, exactly 64, two and four states per lane; n = 2 and 3."""
    run_case(pkg, m, n, 40, 130)


@pytest.mark.parametrize("T", [1, 3, 5, 6, 7, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_frame_lengths(pkg, T):
    """T < m (the state wraps more than once), T = m, the edges of an output word, a 64-step chunk
    and a 1,024-step staging segment; 1,024 / 1,025 is also where m = 6 leaves LDS."""
    run_case(pkg, 6, 2, T, 65 if T < 1000 else 9, seed=T)


@pytest.mark.parametrize("m,n,T", [(8, 3, 1), (8, 2, 7), (8, 3, 256), (8, 3, 257), (7, 2, 512), (7, 2, 513)])
def test_frame_lengths_above_64_states(pkg, m, n, T):
    """T < m, and the two T either side of the LDS / workspace threshold for m = 8 and m = 7."""
    ws = pkg.lib().cvd_viterbi_tailbiting_workspace_bytes
    if T > 8:
        assert (ws(n, m, T, 9, 0) == 0) == (T % 2 == 0)
    run_case(pkg, m, n, T, 9 if T > 8 else 65, seed=T)


@pytest.mark.parametrize("F,T", [(1, 40), (63, 40), (64, 40), (65, 40), (130, 40), (8192 + 70, 16)])
def test_frame_counts(pkg, F, T):
    """One frame, the edges of 64, and more frames than the grid of 8,192 waves, so that a wave
    takes a second frame."""
    run_case(pkg, 6, 2, T, F, seed=F)


# ── laps: the condition on the inputs is asserted on the reference alone ──
LAPS_SEED = 5


@functools.lru_cache(maxsize=None)
def laps_inputs(T):
    gen = gen_of(6, 2)
    capbits, offsets, _ = tailbiting_capture(2, 6, gen, T, 400, 2 * T, 0, LAPS_SEED + T)
    return gen, capbits, offsets


@functools.lru_cache(maxsize=None)
def laps_reference(T, laps):
    gen, capbits, offsets = laps_inputs(T)
    return reference(2, 6, gen, capbits, offsets, T, laps)


def test_laps_inputs_cover_every_outcome():
    """No GPU is consulted: over T = 40 and T = 6 with the default I = 4 the reference produces
    every status, laps 1, 2 and 3, a frame that ran all four laps and one that stopped at lap >= 2
    because E repeated."""
    recs = [laps_reference(T, 4) for T in (40, 6)]
    status = np.concatenate([r[1][:, 3] for r in recs])
    laps = np.concatenate([r[1][:, 6] for r in recs])
    repeated = np.concatenate([r[2] for r in recs])
    assert set(status.tolist()) == {0, 2, 3}
    assert {1, 2, 3, 4} <= set(laps.tolist())
    assert (repeated & (laps >= 2) & (laps < 4)).any()
    # more laps leave fewer frames without a tail-biting best path
    bad = [int((laps_reference(40, I)[1][:, 3] != 0).sum()) for I in (1, 2, 4, 8)]
    assert bad[0] > bad[1] >= bad[2] >= bad[3]


@pytest.mark.parametrize("T", [40, 6])
@pytest.mark.parametrize("laps", [1, 2, 4, 8, None])
def test_laps(pkg, T, laps):
    gen, capbits, offsets = laps_inputs(T)
    res = pkg.decode_frames_tailbiting(2, 6, gen, capbits, T, max_laps=laps)
    want_bits, want_rec, _ = laps_reference(T, laps or 4)
    check(res, want_bits, want_rec, T)
    assert int(res["laps"].max()) <= (laps or 4)


@pytest.mark.parametrize("extra", [0, 1, -3])
@pytest.mark.parametrize("format", ["bytes", "lsb", "msb"])
def test_strides_and_formats(pkg, extra, format):
    """stride n T + 1 walks every bit residue mod 32 over 65 frames, n T - 3 overlaps."""
    run_case(pkg, 6, 2, 40, 65, stride_extra=extra, format=format, seed=7)


@pytest.mark.parametrize("format", ["bytes", "lsb"])
def test_offsets(pkg, format):
    """Unsorted offsets with a duplicate, a negative one, one frame ending exactly at nbits and one
    ending a bit past it: the skipped frames' records and zero rows."""
    m, n, T, F = 6, 2, 40, 20
    gen = gen_of(m, n)
    stride = n * T + 1
    capbits, at, _ = tailbiting_capture(n, m, gen, T, F, stride, 3, 31)
    nbits = len(capbits)
    assert at[-1] + n * T == nbits
    offsets = np.array([at[7], at[0], at[19], -1, at[7], at[19] + 1, at[12], -(1 << 40), nbits, (1 << 62), at[1]],
                       dtype=np.int64)
    ok = np.array([1, 1, 1, 0, 1, 0, 1, 0, 0, 0, 1], dtype=bool)
    cap = as_capture(capbits, format)
    res = pkg.decode_frames_tailbiting(n, m, gen, cap, T, offsets=offsets, format=format, nbits=nbits)
    want_bits = np.zeros((len(offsets), 4 * ((T + 31) // 32)), dtype=np.uint8)
    want_rec = np.tile(np.array(SKIPPED, dtype=np.int64), (len(offsets), 1))
    want_bits[ok], want_rec[ok], _ = reference(n, m, gen, capbits, offsets[ok], T, 4)
    check(res, want_bits, want_rec, T)
    assert res["decoded"] + res["skipped"] == res["F"] == len(offsets) and res["skipped"] == 5
    got = res["frames"].cpu().numpy()
    assert (got[~ok] == SKIPPED).all() and not res["bits"].cpu().numpy()[~ok].any()
    # offsets as a device tensor
    again = pkg.decode_frames_tailbiting(n, m, gen, cap, T, offsets=torch.from_numpy(offsets).to(res["bits"].device),
                                         format=format, nbits=nbits)
    assert torch.equal(again["bits"], res["bits"]) and torch.equal(again["frames"], res["frames"])


@pytest.mark.parametrize("T", [99, 100])
@pytest.mark.parametrize("spec", ["dvb:3/4", "dvb:7/8"])
def test_punctured(pkg, spec, T):
    """The period does and does not divide T; every lap restarts the pattern at column 0."""
    m, n, F = 6, 2, 65
    gen = [[[(g >> (m - d)) & 1 for d in range(m + 1)]] for g in (0o171, 0o133)]
    keep = pkg.puncture_pattern(spec, n)
    span = pkg.punctured_bits(T, keep)
    capbits, offsets, _ = tailbiting_capture(n, m, gen, T, F, span + 5, 3, 19, p=0.01, keep=keep)
    res = pkg.decode_frames_tailbiting(n, m, gen, capbits, T, F=F, start=3, stride=span + 5, keep=spec)
    want_bits, want_rec, _ = reference(n, m, gen, capbits, offsets, T, 4, keep=keep)
    assert (want_rec[:, 5] == span).all()
    check(res, want_bits, want_rec, T)


def test_punctured_with_every_bit_kept_equals_hard(pkg):
    m, n, T, F = 6, 2, 40, 65
    gen = gen_of(m, n)
    capbits, _, _ = tailbiting_capture(n, m, gen, T, F, n * T + 1, 3, 53)
    hard = pkg.decode_frames_tailbiting(n, m, gen, capbits, T, F=F, start=3, stride=n * T + 1)
    for keep in ([3], [3, 3, 3]):
        full = pkg.decode_frames_tailbiting(n, m, gen, capbits, T, F=F, start=3, stride=n * T + 1, keep=keep)
        assert torch.equal(full["bits"], hard["bits"]) and torch.equal(full["frames"], hard["frames"])
        assert {k: v for k, v in full.items() if not isinstance(v, torch.Tensor)} == \
            {k: v for k, v in hard.items() if not isinstance(v, torch.Tensor)}


def soft_tailbiting(n, m, gen, T, F, seed):
    """A soft capture of F tail-biting frames behind 3 junk values: noisy confidences with +-127,
    -128, zeros and, as frame 2, a frame of zeros only."""
    rng = np.random.default_rng(seed)
    capbits, offsets, _ = tailbiting_capture(n, m, gen, T, F, n * T, 3, seed)
    v = (2 * capbits.astype(np.int64) - 1) * rng.integers(1, 128, size=len(capbits))
    v[rng.random(len(v)) < 0.1] = 0
    v[rng.random(len(v)) < 0.05] = 127
    v[rng.random(len(v)) < 0.05] = -127
    v[rng.random(len(v)) < 0.05] = -128
    if F > 2:
        v[offsets[2]:offsets[2] + n * T] = 0
    return v.astype(np.int8), offsets


@pytest.mark.parametrize("m,n,T", [(6, 2, 40), (6, 2, 1025), (6, 3, 40), (8, 3, 40), (2, 2, 40)])
def test_soft_frames(pkg, m, n, T):
    """The frame of zeros ties at every step, so its bits follow from the tie rule alone."""
    gen, F = gen_of(m, n), 65 if T < 1000 else 5
    soft, offsets = soft_tailbiting(n, m, gen, T, F, 23)
    for laps in (None, 1):
        res = pkg.decode_frames_tailbiting_soft(n, m, gen, soft, T, F=F, start=3, max_laps=laps)
        want_bits, want_rec, _ = reference(n, m, gen, None, offsets, T, laps or 4, soft=soft)
        check(res, want_bits, want_rec, T)
    assert want_rec[2].tolist() == [0, 0, 0, 0, 0, 0, 1, 0] and not want_bits[2].any()


@pytest.mark.parametrize("A", [1, 50, 127])
def test_soft_equals_hard_on_signs(pkg, A):
    m, n, T, F = 6, 2, 40, 130
    gen = gen_of(m, n)
    capbits, _, _ = tailbiting_capture(n, m, gen, T, F, n * T + 1, 3, 29)
    hard = pkg.decode_frames_tailbiting(n, m, gen, capbits, T, F=F, start=3, stride=n * T + 1)
    soft = pkg.decode_frames_tailbiting_soft(n, m, gen, pkg.soft_from_bits(capbits, A), T, F=F, start=3,
                                             stride=n * T + 1)
    assert torch.equal(soft["bits"], hard["bits"])
    assert torch.equal(soft["errors"], hard["errors"]) and torch.equal(soft["distance"], A * hard["errors"])
    assert (soft["counted"] == n * T).all()
    assert torch.equal(soft["frames"][:, 1:4], hard["frames"][:, 1:4]) and torch.equal(soft["laps"], hard["laps"])
    assert soft["total_distance"] == A * hard["total_errors"] and soft["ber"] == hard["ber"]
    assert (soft["fallback"], soft["open"], soft["total_laps"]) == (hard["fallback"], hard["open"], hard["total_laps"])
    assert len(set(hard["status"].cpu().tolist())) > 1     # not only frames of status 0


def test_largest_frame(pkg):
    """T = 65536, m = 8, n = 3, every value +-127: the doubled soft metric reaches 127 * 3 * 65536."""
    m, n, T = 8, 3, 65536
    gen = gen_of(m, n)
    capbits, offsets, _ = tailbiting_capture(n, m, gen, T, 1, n * T, 0, 37, p=0.05)
    soft = pkg.soft_from_bits(capbits, 127)
    res = pkg.decode_frames_tailbiting_soft(n, m, gen, soft, T)
    want_bits, want_rec, _ = reference(n, m, gen, None, offsets, T, 4, soft=soft)
    check(res, want_bits, want_rec, T)
    assert want_rec[0, 5] == n * T and want_rec[0, 0] == 127 * want_rec[0, 4] > 127 * 5000


def test_one_lap_equals_decode_frames_any_any(pkg):
    """The header's consistency rule: with I = 1 the frames of status 0 or 3 have the row, the
    distance and the states of decode_frames(start_state=None, end_state=None)."""
    gen, capbits, offsets = laps_inputs(40)
    want = laps_reference(40, 1)[1]
    same = (want[:, 3] == 0) | (want[:, 3] == 3)
    assert 4 * same.sum() >= len(want) and (~same).any()
    tb = pkg.decode_frames_tailbiting(2, 6, gen, capbits, 40, max_laps=1)
    free = pkg.decode_frames(2, 6, gen, capbits, 40, start_state=None, end_state=None)
    sel = torch.from_numpy(np.flatnonzero(same)).to(tb["bits"].device)
    assert np.array_equal(tb["status"].cpu().numpy(), want[:, 3])
    assert torch.equal(tb["bits"][sel], free["bits"][sel])
    assert torch.equal(tb["frames"][sel, :3], free["frames"][sel, :3])


def wrong_frames(rows, u):
    return int((rows != pack_rows(u.astype(np.uint8))).any(axis=1).sum())


def test_fewer_wrong_frames_than_decode_frames(pkg):
    """What the feature is for: (133,171,165), T = 40, p = 0.08.  The reference says so first."""
    m, n, T, F = 6, 3, 40, 400
    gen = gen_of(m, n)
    capbits, offsets, u = tailbiting_capture(n, m, gen, T, F, n * T, 0, 61, p=0.08)
    want_bits, want_rec, _ = reference(n, m, gen, capbits, offsets, T, 4)
    y = received_words(capbits, offsets, frame_positions(n, T)[0])
    want_free = pack_rows(ref_any_any(n, m, gen, hard_cost(n, y)))
    assert wrong_frames(want_bits, u) < wrong_frames(want_free, u)
    tb = pkg.decode_frames_tailbiting(n, m, gen, capbits, T)
    free = pkg.decode_frames(n, m, gen, capbits, T, start_state=None, end_state=None)
    check(tb, want_bits, want_rec, T)
    assert np.array_equal(free["bits"].cpu().numpy(), want_free)
    bad_tb, bad_free = wrong_frames(tb["bits"].cpu().numpy(), u), wrong_frames(free["bits"].cpu().numpy(), u)
    print(f"frames with a wrong information bit: tail-biting {bad_tb}, decode_frames(None, None) {bad_free} of {F}")
    assert bad_tb < bad_free


@pytest.mark.parametrize("T", [40, 128])
def test_noise_free_frames(pkg, T):
    m, n, F = 6, 3, 65
    gen = gen_of(m, n)
    capbits, offsets, u = tailbiting_capture(n, m, gen, T, F, n * T, 3, 67, p=0.0)
    state = wrap_state(m, u)
    want_rec = np.stack([0 * state, state, state, 0 * state, 0 * state, 0 * state + n * T, 0 * state + 1, 0 * state],
                        axis=1)
    ref_bits, ref_rec, _ = reference(n, m, gen, capbits, offsets, T, 4)
    assert np.array_equal(ref_bits, pack_rows(u.astype(np.uint8))) and np.array_equal(ref_rec, want_rec)
    res = pkg.decode_frames_tailbiting(n, m, gen, capbits, T, F=F, start=3)
    check(res, ref_bits, ref_rec, T)


def test_same_result_on_every_launch(pkg, monkeypatch):
    """Two calls, another stream, another grid (130 frames on 7 waves) and the other placement of
    the decision words (the workspace instead of LDS) all give the same result."""
    m, n, T, F = 6, 2, 40, 130
    gen = gen_of(m, n)
    capbits, _, _ = tailbiting_capture(n, m, gen, T, F, n * T, 3, 41)
    cap = torch.from_numpy(np.concatenate([capbits, np.zeros(-len(capbits) % 16, dtype=np.uint8)])).cuda()
    kw = dict(F=F, start=3, nbits=len(capbits))
    first = pkg.decode_frames_tailbiting(n, m, gen, cap, T, **kw)
    others = [pkg.decode_frames_tailbiting(n, m, gen, cap, T, **kw)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        others.append(pkg.decode_frames_tailbiting(n, m, gen, cap, T, **kw))
    stream.synchronize()
    ws = pkg.lib().cvd_viterbi_tailbiting_workspace_bytes
    assert ws(n, m, T, F, 0) == 0
    monkeypatch.setenv("CVD_TAILBITE_WAVES", "7")
    others.append(pkg.decode_frames_tailbiting(n, m, gen, cap, T, **kw))
    monkeypatch.setenv("CVD_TAILBITE_LDS_BYTES", "1")
    assert ws(n, m, T, F, 0) == 7 * 64 * 8
    others.append(pkg.decode_frames_tailbiting(n, m, gen, cap, T, **kw))
    monkeypatch.delenv("CVD_TAILBITE_WAVES")
    assert ws(n, m, T, F, 0) == F * 64 * 8
    others.append(pkg.decode_frames_tailbiting(n, m, gen, cap, T, **kw))
    for other in others:
        assert torch.equal(other["bits"], first["bits"]) and torch.equal(other["frames"], first["frames"])
        assert {k: v for k, v in other.items() if not isinstance(v, torch.Tensor)} == \
            {k: v for k, v in first.items() if not isinstance(v, torch.Tensor)}


def test_argument_errors(pkg):
    gen = gen_of(6, 2)
    cap = np.zeros(1000, dtype=np.uint8)
    for kw in (dict(T=0), dict(T=65537), dict(T=100, F=6), dict(T=100, start=-1), dict(T=100, stride=0),
               dict(T=100, max_laps=0), dict(T=100, max_laps=9), dict(T=100, offsets=np.zeros(3), F=4)):
        with pytest.raises((ValueError, TypeError)):
            pkg.decode_frames_tailbiting(2, 6, gen, cap, **kw)
    none = pkg.decode_frames_tailbiting(2, 6, gen, cap, 100, F=0)
    assert none["bits"].shape == (0, 16) and none["frames"].shape == (0, 8) and none["decoded"] == 0
    assert (none["fallback"], none["open"], none["total_laps"], none["words"]) == (0, 0, 0, 4)
    assert pkg.decode_frames_tailbiting(2, 6, gen, cap, 100)["F"] == 5      # as many as fit
    with pytest.raises(pkg._lib.CvdError, match="viterbi_decode_frames_tailbiting"):
        pkg.decode_frames_tailbiting(2, 9, [[[1] * 10], [[1, 0, 1, 1, 1, 0, 0, 0, 1, 1]]], cap, 100)


def test_decode_cli_tail_biting(pkg, tmp_path):
    """decode --frame 40 --tail-biting in a fresh process: the .npy and the CSV rows, laps among
    them, equal the Python call's; without --tail-biting the CSV keeps its header."""
    m, n, T, F = 6, 2, 40, 30
    gen = gen_of(m, n)
    stride = n * T + 7
    capbits, offsets, _ = tailbiting_capture(n, m, gen, T, F, stride, 3, 43)
    npy, out = str(tmp_path / "cap.npy"), str(tmp_path / "res")
    np.save(npy, capbits)
    pkg_name = os.path.basename(os.path.dirname(pkg.__file__))
    base = [sys.executable, "-m", pkg_name, "decode", "--code", "oct:133,171", "--input", npy, "--start", "3",
            "--frame", str(T), "--frame-stride", str(stride), "--save-dir", out]
    run = subprocess.run(base + ["--tail-biting", "--laps", "2"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    want = pkg.decode_frames_tailbiting(n, m, gen, capbits, T, start=3, stride=stride, max_laps=2)
    assert want["F"] == F
    got = np.load(os.path.join(out, "decoded.npy"))
    assert got.dtype == np.uint8 and got.shape == (F, 4 * 2) and np.array_equal(got, want["bits"].cpu().numpy())
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    old_header = ["frame", "offset", "status", "distance", "errors", "counted", "start_state", "end_state"]
    assert rows[0] == old_header + ["laps"]
    rec = want["frames"].cpu().numpy()
    assert [[int(x) for x in r] for r in rows[1:]] == \
        [[i, int(offsets[i]), rec[i, 3], rec[i, 0], rec[i, 4], rec[i, 5], rec[i, 1], rec[i, 2], rec[i, 6]]
         for i in range(F)]
    assert f"Decoded {F} frames of {T} steps (0 skipped)" in run.stdout
    assert f"p = {want['ber']!r}" in run.stdout
    assert f"Tail-biting: {want['fallback']} frames fell back" in run.stdout
    assert f"{want['total_laps'] / F:.3f} laps per frame" in run.stdout
    run = subprocess.run(base + ["--end-state", "any"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == old_header and len(rows) == F + 1 and all(len(r) == 8 for r in rows)
    assert "Tail-biting" not in run.stdout

"""cvd_viterbi_decode_frames, _punctured and _soft on the GPU against a sequential numpy decoder
written from the contract in include/cvd.h (unnormalised integer metrics with a big constant
for +inf, ties keep b = 0, the lowest-index best end state): the rows of bits, all six fields
of every frame's record and all six totals are compared exactly."""
import csv
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


def encode(n, m, gen, u):
    """Output words [F, T] of the input bits u [F, T] from state 0."""
    F, T = u.shape
    past = np.concatenate([np.zeros((F, m), dtype=np.int64), u], axis=1)     # u_{t-d} at column m + t - d
    y = np.zeros((F, T), dtype=np.int64)
    for j in range(n):
        bit = np.zeros((F, T), dtype=np.int64)
        for d in range(m + 1):
            if gen[j][0][d]:
                bit ^= past[:, m - d:m - d + T]
        y |= bit << j
    return y


def ref_decode(n, m, gen, cost, start_state, end_state):
    """The contract's decoder over cost[F, T, 2^n] (the metric of output word o at step t):
    bits [F, T], distance, s_0, s_T [F] and the traced path's output words [F, T]."""
    F, T, _ = cost.shape
    S = 1 << m
    ps, out = trellis(n, m, gen)
    D = np.zeros((F, S), dtype=np.int64)
    if start_state is not None:
        D[:] = BIG
        D[:, start_state] = 0
    dec = np.zeros((F, T, S), dtype=bool)
    for t in range(T):
        c0 = D[:, ps[0]] + cost[:, t][:, out[0]]
        c1 = D[:, ps[1]] + cost[:, t][:, out[1]]
        dec[:, t] = c1 < c0                              # ties keep b = 0
        D = np.minimum(c0, c1)
    rows = np.arange(F)
    sT = np.argmin(D, axis=1) if end_state is None else np.full(F, end_state)   # argmin: the lowest index
    dist = D[rows, sT]
    assert (dist < BIG).all()
    bits = np.zeros((F, T), dtype=np.uint8)
    words = np.zeros((F, T), dtype=np.int64)
    s = sT.copy()
    for t in range(T - 1, -1, -1):
        bits[:, t] = s & 1
        b = dec[rows, t, s].astype(np.int64)
        words[:, t] = out[b, s]
        s = (s >> 1) | (b << (m - 1))
    return bits, dist, s, sT, words


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


def reference(n, m, gen, capbits, offsets, T, ss, es, keep=None, soft=None):
    """What decode_frames / decode_frames_soft must return for frames at `offsets` (all inside the
    capture): bits uint8 [F, 4w], frames int64 [F, 6]."""
    pos, masks, span = frame_positions(n, T, keep)
    if soft is None:
        y = received_words(capbits, offsets, pos)
        bits, dist, s0, sT, words = ref_decode(n, m, gen, hard_cost(n, y, None if keep is None else masks), ss, es)
        errors, counted = dist, np.full(len(offsets), span)
    else:
        v = soft[offsets[:, None, None] + pos[None]]
        bits, dist, s0, sT, words = ref_decode(n, m, gen, soft_cost(n, v), ss, es)
        _, nz, one = soft_values(n, v)
        path = ((words[:, :, None] >> np.arange(n)[None, None, :]) & 1).astype(bool)
        errors, counted = (nz & (one != path)).sum(axis=(1, 2)), nz.sum(axis=(1, 2))
    rec = np.stack([dist, s0, sT, np.zeros_like(dist), errors, counted], axis=1)
    return pack_rows(bits), rec


def check(res, want_bits, want_rec, T):
    """The GPU result against the reference's rows and records, and the totals against their sums."""
    got_bits, got_rec = res["bits"].cpu().numpy(), res["frames"].cpu().numpy().astype(np.int64)
    assert got_bits.dtype == np.uint8 and got_bits.shape == want_bits.shape
    assert np.array_equal(got_rec, want_rec), np.argwhere(got_rec != want_rec)[:10]
    assert np.array_equal(got_bits, want_bits), np.argwhere(got_bits != want_bits)[:10]
    ok = want_rec[:, 3] == 0
    assert res["T"] == T and res["F"] == len(want_rec) and res["words"] == (T + 31) // 32
    assert (res["total_distance"], res["decoded"], res["skipped"], res["total_errors"], res["total_counted"]) == \
        (int(want_rec[ok, 0].sum()), int(ok.sum()), int((~ok).sum()), int(want_rec[ok, 4].sum()),
         int(want_rec[ok, 5].sum()))
    for i, name in enumerate(["distance", "start_states", "end_states", "status", "errors", "counted"]):
        assert np.array_equal(res[name].cpu().numpy(), want_rec[:, i])
    assert res["ber"] == (res["total_errors"] / res["total_counted"] if res["total_counted"] else 0.0)


def framed_capture(n, m, gen, T, F, stride, start, seed, p=0.08, keep=None, tail_burst=0):
    """A bit array holding F terminated frames (random data, m zero tail bits, from state 0) at
    start + f stride, sent through a BSC(p); tail_burst: flip probability 1/2 over the last
    tail_burst steps' bits."""
    rng = np.random.default_rng(seed)
    pos, _, span = frame_positions(n, T, keep)
    u = rng.integers(0, 2, size=(F, T), dtype=np.int64)
    u[:, max(0, T - m):] = 0
    y = encode(n, m, gen, u)
    nbits = start + (F - 1) * stride + span
    capbits = rng.integers(0, 2, size=nbits, dtype=np.uint8)
    flip = rng.random((F, T, n)) < p
    if tail_burst:
        flip[:, T - tail_burst:] = rng.random((F, tail_burst, n)) < 0.5
    for f in range(F):                                   # in order: an overlapping frame overwrites its neighbour
        for j in range(n):
            sent = pos[:, j] >= 0
            capbits[start + f * stride + pos[sent, j]] = ((y[f, sent] >> j) & 1) ^ flip[f, sent, j]
    return capbits, start + stride * np.arange(F, dtype=np.int64)


def run_case(pkg, m, n, T, F, stride_extra=0, format="bytes", ss=0, es=0, seed=1):
    gen = gen_of(m, n)
    stride = n * T + stride_extra
    capbits, offsets = framed_capture(n, m, gen, T, F, stride, 3, seed)
    res = pkg.decode_frames(n, m, gen, as_capture(capbits, format), T, F=F, start=3, stride=stride, start_state=ss,
                            end_state=es, format=format, nbits=len(capbits))
    want_bits, want_rec = reference(n, m, gen, capbits, offsets, T, ss, es)
    check(res, want_bits, want_rec, T)
    return res, want_rec


@pytest.mark.parametrize("m,n", sorted(OCT))
def test_code_shapes(pkg, m, n):
    """Fewer than 64 states, exactly 64, two and four states per lane; n = 2 and 3."""
    run_case(pkg, m, n, 200, 65)


@pytest.mark.parametrize("T", [6, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_frame_lengths(pkg, T):
    """T = m, and the edges of an output word, a 64-step chunk and a 1,024-step staging segment."""
    run_case(pkg, 6, 2, T, 65, seed=T)


@pytest.mark.parametrize("F,T", [(1, 200), (63, 200), (64, 200), (65, 200), (130, 200), (8192 + 70, 16)])
def test_frame_counts(pkg, F, T):
    """One frame, the edges of the traceback's 64 frames per wave, and more frames than the forward
    kernel's grid of 8,192 waves."""
    run_case(pkg, 6, 2, T, F, seed=F)


@pytest.mark.parametrize("extra", [0, 1, -3])
@pytest.mark.parametrize("format", ["bytes", "lsb", "msb"])
def test_strides_and_formats(pkg, extra, format):
    """stride n T + 1 walks every bit residue mod 32 over 65 frames, n T - 3 overlaps."""
    run_case(pkg, 6, 2, 200, 65, stride_extra=extra, format=format, seed=7)


@pytest.mark.parametrize("ss,es", [(0, 0), (None, 0), (0, None), (None, None), (5, 9)])
def test_boundary_conditions(pkg, ss, es):
    res, want = run_case(pkg, 6, 2, 200, 65, ss=ss, es=es, seed=11)
    if ss is not None:
        assert (res["start_states"].cpu().numpy() == ss).all()
    if es is not None:
        assert (res["end_states"].cpu().numpy() == es).all()


def test_short_frames_with_one_state_fixed(pkg):
    """T < m with one boundary fixed: states of infinite metric exist at the end of the frame."""
    run_case(pkg, 6, 2, 3, 65, ss=0, es=None, seed=13)
    run_case(pkg, 6, 2, 3, 65, ss=None, es=9, seed=13)
    run_case(pkg, 8, 3, 1, 65, ss=77, es=None, seed=13)


BURST_SEED = 3


def test_termination_changes_the_answer(pkg):
    """A burst over the last 2 m steps: knowing the end state changes the decoded bits.  The
    reference itself must say so before the GPU is asked."""
    m, n, T, F = 6, 2, 96, 65
    gen = gen_of(m, n)
    capbits, offsets = framed_capture(n, m, gen, T, F, n * T, 0, BURST_SEED, tail_burst=2 * m)
    term = reference(n, m, gen, capbits, offsets, T, 0, 0)
    free = reference(n, m, gen, capbits, offsets, T, None, None)
    assert (term[0] != free[0]).any(axis=1).sum() >= 1
    assert (free[1][:, 0] <= term[1][:, 0]).all()
    for (ss, es), want in (((0, 0), term), ((None, None), free)):
        res = pkg.decode_frames(n, m, gen, capbits, T, start_state=ss, end_state=es)
        assert res["F"] == F
        check(res, want[0], want[1], T)


def unpack_row(row, T):
    return np.unpackbits(row, bitorder="little")[:T]


@pytest.mark.parametrize("T", [100, 1025])
def test_equals_decode_capture(pkg, T):
    m, n, F = 6, 2, 5
    gen = gen_of(m, n)
    capbits, offsets = framed_capture(n, m, gen, T, F, n * T + 5, 3, 17)
    res = pkg.decode_frames(n, m, gen, capbits, T, F=F, start=3, stride=n * T + 5, start_state=None, end_state=None)
    bits, rec = res["bits"].cpu().numpy(), res["frames"].cpu().numpy()
    for f in range(F):
        one = pkg.decode_capture(n, m, gen, capbits, start=int(offsets[f]), T=T)
        assert np.array_equal(one["bits"].cpu().numpy(), bits[f])
        assert (one["errors"], one["start_state"], one["end_state"]) == (rec[f, 0], rec[f, 1], rec[f, 2])


@pytest.mark.parametrize("T", [99, 100])
def test_equals_decode_capture_punctured(pkg, T):
    """dvb:3/4 at a multiple of the period and at a non-multiple; against the numpy decoder too."""
    m, n, F = 6, 2, 5
    gen = [[[(g >> (m - d)) & 1 for d in range(m + 1)]] for g in (0o171, 0o133)]
    keep = pkg.puncture_pattern("dvb:3/4", n)
    span = pkg.punctured_bits(T, keep)
    capbits, offsets = framed_capture(n, m, gen, T, F, span + 5, 3, 19, keep=keep)
    for ss, es in ((None, None), (0, 0)):
        res = pkg.decode_frames(n, m, gen, capbits, T, F=F, start=3, stride=span + 5, start_state=ss, end_state=es,
                                keep="dvb:3/4")
        want_bits, want_rec = reference(n, m, gen, capbits, offsets, T, ss, es, keep=keep)
        assert (want_rec[:, 5] == span).all()
        check(res, want_bits, want_rec, T)
    res = pkg.decode_frames(n, m, gen, capbits, T, F=F, start=3, stride=span + 5, start_state=None, end_state=None,
                            keep=keep)
    bits, rec = res["bits"].cpu().numpy(), res["frames"].cpu().numpy()
    for f in range(F):
        one = pkg.decode_capture_punctured(n, m, gen, keep, capbits, start=int(offsets[f]), T=T)
        assert np.array_equal(one["bits"].cpu().numpy(), bits[f])
        assert (one["errors"], one["start_state"], one["end_state"], one["capture_bits"]) == \
            (rec[f, 0], rec[f, 1], rec[f, 2], rec[f, 5])


def soft_frames(n, m, gen, T, F, seed):
    """A soft capture of F frames behind 3 junk values: noisy confidences with +-127, -128, zeros
    and, as frame 2, a frame of zeros only."""
    rng = np.random.default_rng(seed)
    capbits, offsets = framed_capture(n, m, gen, T, F, n * T, 3, seed, p=0.05)
    v = (2 * capbits.astype(np.int64) - 1) * rng.integers(1, 128, size=len(capbits))
    v[rng.random(len(v)) < 0.1] = 0
    v[rng.random(len(v)) < 0.05] = 127
    v[rng.random(len(v)) < 0.05] = -127
    v[rng.random(len(v)) < 0.05] = -128
    if F > 2:
        v[offsets[2]:offsets[2] + n * T] = 0
    return v.astype(np.int8), offsets


@pytest.mark.parametrize("m,n,T", [(6, 2, 100), (6, 2, 1025), (8, 3, 100), (2, 2, 100)])
def test_soft_frames(pkg, m, n, T):
    """Against the numpy decoder and against decode_capture_soft; the frame of zeros ties at every
    step, so its bits follow from the tie rule alone."""
    gen, F = gen_of(m, n), 5
    soft, offsets = soft_frames(n, m, gen, T, F, 23)
    for ss, es in ((0, 0), (None, None)):
        res = pkg.decode_frames_soft(n, m, gen, soft, T, F=F, start=3, start_state=ss, end_state=es)
        want_bits, want_rec = reference(n, m, gen, None, offsets, T, ss, es, soft=soft)
        check(res, want_bits, want_rec, T)
    bits, rec = res["bits"].cpu().numpy(), res["frames"].cpu().numpy()
    assert rec[2].tolist() == [0, 0, 0, 0, 0, 0] and not bits[2].any()
    for f in range(F):
        one = pkg.decode_capture_soft(n, m, gen, soft, start=int(offsets[f]), T=T)
        assert np.array_equal(one["bits"].cpu().numpy(), bits[f])
        assert (one["metric"], one["start_state"], one["end_state"], one["errors"], n * T - one["erasures"]) == \
            tuple(rec[f, [0, 1, 2, 4, 5]])


@pytest.mark.parametrize("A", [1, 50, 127])
def test_soft_equals_hard_on_signs(pkg, A):
    m, n, T, F = 6, 2, 200, 65
    gen = gen_of(m, n)
    capbits, _ = framed_capture(n, m, gen, T, F, n * T + 1, 3, 29)
    hard = pkg.decode_frames(n, m, gen, capbits, T, F=F, start=3, stride=n * T + 1)
    soft = pkg.decode_frames_soft(n, m, gen, pkg.soft_from_bits(capbits, A), T, F=F, start=3, stride=n * T + 1)
    assert torch.equal(soft["bits"], hard["bits"])
    assert torch.equal(soft["errors"], hard["errors"]) and torch.equal(soft["distance"], A * hard["errors"])
    assert (soft["counted"] == n * T).all()
    assert torch.equal(soft["frames"][:, 1:4], hard["frames"][:, 1:4])
    assert soft["total_distance"] == A * hard["total_errors"] and soft["ber"] == hard["ber"]


@pytest.mark.parametrize("format", ["bytes", "lsb"])
def test_offsets(pkg, format):
    """Unsorted offsets with a duplicate, a negative one, one frame ending exactly at nbits and one
    ending a bit past it; the capture buffer ends at nbits rounded up to 16 bytes."""
    m, n, T, F = 6, 2, 200, 20
    gen = gen_of(m, n)
    stride = n * T + 1
    capbits, at = framed_capture(n, m, gen, T, F, stride, 3, 31)
    nbits = len(capbits)
    assert at[-1] + n * T == nbits
    offsets = np.array([at[7], at[0], at[19], -1, at[7], at[19] + 1, at[12], -(1 << 40), nbits, (1 << 62), at[1]],
                       dtype=np.int64)
    ok = np.array([1, 1, 1, 0, 1, 0, 1, 0, 0, 0, 1], dtype=bool)
    cap = as_capture(capbits, format)
    res = pkg.decode_frames(n, m, gen, cap, T, offsets=offsets, format=format, nbits=nbits)
    want_bits = np.zeros((len(offsets), 4 * ((T + 31) // 32)), dtype=np.uint8)
    want_rec = np.tile(np.array([0, -1, -1, 1, 0, 0], dtype=np.int64), (len(offsets), 1))
    want_bits[ok], want_rec[ok] = reference(n, m, gen, capbits, offsets[ok], T, 0, 0)
    check(res, want_bits, want_rec, T)
    assert res["decoded"] + res["skipped"] == res["F"] == len(offsets) and res["skipped"] == 5
    # the same frames in stride mode
    strided = pkg.decode_frames(n, m, gen, cap, T, F=F, start=3, stride=stride, format=format, nbits=nbits)
    idx = torch.tensor([7, 0, 19, 7, 12, 1], device=strided["bits"].device)
    sel = torch.tensor(np.flatnonzero(ok), device=strided["bits"].device)
    assert torch.equal(res["bits"][sel], strided["bits"][idx])
    assert torch.equal(res["frames"][sel], strided["frames"][idx])
    # offsets as a device tensor
    again = pkg.decode_frames(n, m, gen, cap, T, offsets=torch.from_numpy(offsets).to(res["bits"].device),
                              format=format, nbits=nbits)
    assert torch.equal(again["bits"], res["bits"]) and torch.equal(again["frames"], res["frames"])


def test_largest_frame(pkg):
    """T = 65536, m = 8, n = 3, every value +-127 with a tenth of the signs flipped: the doubled
    soft metric reaches 127 * 3 * 65536 and the constant that stands for +inf sits above it."""
    m, n, T = 8, 3, 65536
    gen = gen_of(m, n)
    capbits, offsets = framed_capture(n, m, gen, T, 1, n * T, 0, 37, p=0.1)
    soft = pkg.soft_from_bits(capbits, 127)
    res = pkg.decode_frames_soft(n, m, gen, soft, T)
    want_bits, want_rec = reference(n, m, gen, None, offsets, T, 0, 0, soft=soft)
    check(res, want_bits, want_rec, T)
    assert want_rec[0, 5] == n * T and want_rec[0, 0] == 127 * want_rec[0, 4] > 127 * 10000


def test_same_result_on_every_launch(pkg):
    m, n, T, F = 6, 2, 200, 130
    gen = gen_of(m, n)
    capbits, _ = framed_capture(n, m, gen, T, F, n * T, 3, 41)
    cap = torch.from_numpy(np.concatenate([capbits, np.zeros(-len(capbits) % 16, dtype=np.uint8)])).cuda()
    kw = dict(F=F, start=3, nbits=len(capbits))
    first = pkg.decode_frames(n, m, gen, cap, T, **kw)
    second = pkg.decode_frames(n, m, gen, cap, T, **kw)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        third = pkg.decode_frames(n, m, gen, cap, T, **kw)
    stream.synchronize()
    for other in (second, third):
        assert torch.equal(other["bits"], first["bits"]) and torch.equal(other["frames"], first["frames"])
        assert {k: v for k, v in other.items() if not isinstance(v, torch.Tensor)} == \
            {k: v for k, v in first.items() if not isinstance(v, torch.Tensor)}


def test_same_result_batch_after_batch(pkg, monkeypatch):
    """The workspace holds a batch of frames; with a small CVD_FRAMES_BATCH_BYTES 130 frames of 200
    steps (2 KiB of decision words each) go through three batches of 64, 64 and 2."""
    m, n, T, F = 6, 2, 200, 130
    gen = gen_of(m, n)
    ws = pkg.lib().cvd_viterbi_frames_workspace_bytes
    capbits, offsets = framed_capture(n, m, gen, T, F, n * T + 1, 3, 47)
    soft, _ = soft_frames(n, m, gen, T, F, 47)
    whole = ws(n, m, T, F, 0)
    assert whole == F * 256 * 8
    monkeypatch.setenv("CVD_FRAMES_BATCH_BYTES", "65536")
    assert ws(n, m, T, F, 0) == ws(n, m, T, F, 1) == 64 * 256 * 8 < whole
    res = pkg.decode_frames(n, m, gen, capbits, T, F=F, start=3, stride=n * T + 1)
    check(res, *reference(n, m, gen, capbits, offsets, T, 0, 0), T)
    res = pkg.decode_frames_soft(n, m, gen, soft, T, F=F, start=3)
    check(res, *reference(n, m, gen, None, 3 + n * T * np.arange(F), T, 0, 0, soft=soft), T)


def test_argument_errors(pkg):
    gen = gen_of(6, 2)
    cap = np.zeros(1000, dtype=np.uint8)
    for kw in (dict(T=0), dict(T=65537), dict(T=100, F=6), dict(T=100, start=-1), dict(T=100, stride=0),
               dict(T=100, start_state=64), dict(T=100, end_state=-1), dict(T=5), dict(T=100, offsets=np.zeros(3), F=4)):
        with pytest.raises((ValueError, TypeError)):
            pkg.decode_frames(2, 6, gen, cap, **kw)
    with pytest.raises(NotImplementedError, match="decode_frames"):
        pkg.decode_frames_soft(2, 6, gen, cap.astype(np.int8), 100, keep="dvb:3/4")
    none = pkg.decode_frames(2, 6, gen, cap, 100, F=0)
    assert none["bits"].shape == (0, 16) and none["frames"].shape == (0, 6) and none["decoded"] == 0
    assert pkg.decode_frames(2, 6, gen, cap, 100)["F"] == 5      # as many as fit


def test_decode_cli_frames(pkg, tmp_path):
    """decode --frame in a fresh process: the .npy and the CSV rows equal the Python call's."""
    m, n, T, F = 6, 2, 100, 9
    gen = gen_of(m, n)
    stride = n * T + 7
    capbits, offsets = framed_capture(n, m, gen, T, F, stride, 3, 43)
    npy, out = str(tmp_path / "cap.npy"), str(tmp_path / "res")
    np.save(npy, capbits)
    pkg_name = os.path.basename(os.path.dirname(pkg.__file__))
    run = subprocess.run([sys.executable, "-m", pkg_name, "decode", "--code", "oct:133,171", "--input", npy, "--start", "3",
                          "--frame", str(T), "--frame-stride", str(stride), "--end-state", "any", "--save-dir", out],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    want = pkg.decode_frames(n, m, gen, capbits, T, start=3, stride=stride, end_state=None)
    assert want["F"] == F
    got = np.load(os.path.join(out, "decoded.npy"))
    assert got.dtype == np.uint8 and got.shape == (F, 4 * 4) and np.array_equal(got, want["bits"].cpu().numpy())
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "offset", "status", "distance", "errors", "counted", "start_state", "end_state"]
    rec = want["frames"].cpu().numpy()
    assert [[int(x) for x in r] for r in rows[1:]] == \
        [[i, int(offsets[i]), rec[i, 3], rec[i, 0], rec[i, 4], rec[i, 5], rec[i, 1], rec[i, 2]] for i in range(F)]
    assert f"Decoded {F} frames of {T} steps (0 skipped)" in run.stdout
    assert f"p = {want['ber']!r}" in run.stdout

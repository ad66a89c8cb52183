"""Every code shape of the three capture decoders: m = 1..8 x n = 2, 3 through cvd_viterbi_decode,
cvd_viterbi_decode_punctured and cvd_viterbi_decode_soft, against the numpy restatements of
test_gpu_decode.py, test_gpu_decode_punctured.py and test_gpu_decode_soft.py (imported, not
restated): bits and every stats entry, exactly.  The other decoder tests run m in {2, 3, 6, 8};
each (m, n) has forward and join kernels of its own in each decoder (m = 7: two states per lane).
One shape, the smallest at which every path of a run is taken: blocks of 1,120 steps (a
1,024-step staging segment, then a 32-step partial chunk), T = 2 * 1120 + 45 (a short last block
that ends in a 45-step chunk), the capture from bit / value 5 (funnel shift and byte offset
unaligned).  Two settings: warm = 40, depth = 64 (a warm-up with a partial chunk), and warm = 0,
depth = 0, where the restatement itself must count a forward rerun and a traceback fix-up in
every case, so the join reruns blocks and fix resolves them."""
import numpy as np
import pytest
import torch

import test_gpu_decode as H
import test_gpu_decode_punctured as P
import test_gpu_decode_soft as S
from test_gpu_capture import raw_capture

pytestmark = pytest.mark.gpu

# taps of delays 0..m as octal digits, delay 0 first: every code has a tap at delay 0 and at delay m
POLYS = {
    (1, 2): "3,1", (1, 3): "3,1,2",
    (2, 2): "7,5", (2, 3): "7,5,7",
    (3, 2): "17,15", (3, 3): "13,15,17",
    (4, 2): "23,35", (4, 3): "25,33,37",
    (5, 2): "53,75", (5, 3): "47,53,75",
    (6, 2): "133,171", (6, 3): "133,145,175",
    (7, 2): "247,371", (7, 3): "225,331,367",
    (8, 2): "561,753", (8, 3): "557,663,711",
}
SHAPES = sorted(POLYS)
START, L = 5, 1120
T = 2 * L + 45
SETTINGS = [(40, 64), (0, 0)]                # warm, depth
KEEP = {2: [3, 2, 1], 3: [7, 1, 6, 2, 5]}    # n = 2: "101/110" as column masks
P_FLIP = 0.05

_CACHE = {}


def gen_of(m, n):
    """gen[j][0][d] of the shape's code."""
    gen = [[[int(c) for c in format(int(g, 8), "0%db" % (m + 1))]] for g in POLYS[m, n].split(",")]
    assert len(gen) == n and any(g[0][0] for g in gen) and any(g[0][m] for g in gen)
    return gen


def sent_bits(tr, rng):
    """[T, n]: the code's outputs over T random input bits from state 0, each flipped with
    probability P_FLIP."""
    u = rng.integers(0, 2, T)
    out = np.zeros(T, np.int64)
    s = 0
    for t in range(T):
        out[t] = tr.out[s, u[t]]
        s = ((s << 1) | int(u[t])) & (tr.S - 1)
    sent = ((out[:, None] >> np.arange(tr.n)) & 1).astype(np.uint8)
    return sent ^ (rng.random(sent.shape) < P_FLIP).astype(np.uint8)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def case(kind, m, n):
    """The capture of a case and its restatement at both settings; built once, not changed."""
    key = (kind, m, n)
    if key not in _CACHE:
        gen = gen_of(m, n)
        rng = np.random.default_rng(1000 * m + n)
        junk, tail = rng.integers(0, 2, START).astype(np.uint8), rng.integers(0, 2, 3).astype(np.uint8)
        if kind == "hard":
            tr = H.Trellis(gen, n, m)
            data = np.concatenate([junk, sent_bits(tr, rng).reshape(-1), tail])
            fwd = frozen(*H.forward(tr, H.symbols(data, n, START, T)))
            want = [H.restatement(tr, data, START, T, L, W, Dp, fwd=fwd) for W, Dp in SETTINGS]
        elif kind == "punctured":
            tr = H.Trellis(gen, n, m)
            keep = KEEP[n]
            mask = P.positions(keep, T)[1]
            data = np.concatenate([junk, sent_bits(tr, rng)[((mask[:, None] >> np.arange(n)) & 1) == 1], tail])
            fwd = frozen(*P.forward(tr, *P.symbols(data, n, keep, START, T)))
            want = [P.restatement(tr, data, keep, START, T, L, W, Dp, fwd=fwd) for W, Dp in SETTINGS]
        else:
            tr = S.SoftTrellis(gen, n, m)
            data = rng.integers(-128, 128, START + n * T + 3).astype(np.int8)
            assert (data[START:START + n * T] == 0).any() and (data[START:START + n * T] == -128).any()
            fwd = frozen(*S.forward(tr, S.values(data, n, START, T)))
            want = [S.restatement(tr, data, START, T, L, W, Dp, fwd=fwd) for W, Dp in SETTINGS]
        frozen(data)
        _CACHE[key] = (gen, data, want)
    return _CACHE[key]


def check_settings(want, decode):
    """decode(warm, depth) against the restatement at each setting."""
    for (W, Dp), w in zip(SETTINGS, want):
        assert w["blocks"] == 3
        if (W, Dp) == (0, 0):
            assert w["forward_reruns"] >= 1 and w["trace_fixups"] >= 1
        H.check(decode(W, Dp), w)


@pytest.mark.parametrize("m,n", SHAPES)
def test_hard(pkg, m, n):
    gen, bits, want = case("hard", m, n)
    cap = torch.from_numpy(raw_capture(bits, "lsb", np.random.default_rng(3))).cuda()
    check_settings(want, lambda W, Dp: pkg.decode_capture(n, m, gen, cap, start=START, T=T, format="lsb",
                                                          nbits=len(bits), block=L, warm=W, depth=Dp))


@pytest.mark.parametrize("m,n", SHAPES)
def test_punctured(pkg, m, n):
    gen, bits, want = case("punctured", m, n)
    keep = KEEP[n]
    assert pkg.puncture_pattern("101/110", 2) == KEEP[2]
    assert want[0]["capture_bits"] == pkg.punctured_bits(T, keep) == len(bits) - START - 3
    cap = torch.from_numpy(raw_capture(bits, "lsb", np.random.default_rng(3))).cuda()
    check_settings(want, lambda W, Dp: pkg.decode_capture_punctured(n, m, gen, keep, cap, start=START, T=T,
                                                                    format="lsb", nbits=len(bits), block=L, warm=W,
                                                                    depth=Dp))


@pytest.mark.parametrize("m,n", SHAPES)
def test_soft(pkg, m, n):
    gen, soft, want = case("soft", m, n)
    cap = torch.from_numpy(soft.copy()).cuda()
    check_settings(want, lambda W, Dp: pkg.decode_capture_soft(n, m, gen, cap, start=START, T=T, block=L, warm=W,
                                                               depth=Dp))

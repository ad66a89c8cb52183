"""Decoding a punctured capture on the GPU: cvd_viterbi_decode_punctured against a numpy
restatement of the header (test_gpu_decode.py's sequential decoder and counter definitions,
extended by a per-step mask and pos(t)), on the C oracle's streams with the kept bits picked
out behind a junk prefix.  Every expected value is exact; no test asserts a statistical
outcome.  The shapes are the smallest at which the pattern-aware forward pass can go wrong:
periods (2, 3, 5, 7) that divide neither a word, a chunk nor a segment, T below a period, a
tail inside a period, blocks and warm-ups that begin in every column, a segment boundary
mid-period, 2^m below, at and above a wavefront's 64 lanes, and n = 3 with 1 to 3 bits a step."""
import csv
import importlib
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from test_gpu_capture import JUNK, SEED, capture_bits, raw_capture, serial_bits
from test_gpu_decode import POP, TMAX, Trellis, check, unpacked
from test_gpu_decode import oracle_case as unpunctured_case

pytestmark = pytest.mark.gpu

CASES = {
    # name: (octal spec, pattern, capture format of its cases)
    "m2": ("oct:7,5", "10/11", "bytes"),                 # 4 states
    "m6_34": ("oct:171,133", "dvb:3/4", "lsb"),          # 64 states, period 3
    "m6_78": ("oct:171,133", "dvb:7/8", "bytes"),        # period 7
    "m8": ("oct:561,753", "dvb:5/6", "msb"),             # 256 states: four per lane, period 5
    "m3n3": ("oct:13,15,17", [7, 1, 6, 2, 5], "msb"),    # n = 3: 1 to 3 bits per step
}


# ───────────────────────────── numpy restatement ────────────────────────────

def positions(keep, T):
    """(pos(t) - start for t = 0..T, keep[t mod period] for t = 0..T-1) of include/cvd.h."""
    keep = np.asarray(keep, np.int64)
    period = len(keep)
    pre = np.concatenate([[0], np.cumsum(POP[keep])])
    t = np.arange(T + 1, dtype=np.int64)
    return (t // period) * pre[period] + pre[t % period], keep[t[:T] % period]


def symbols(bits, n, keep, start, T):
    """(y_t, mask_t): the kept outputs of step t, j ascending, are capture bits pos(t),
    pos(t) + 1, ...; y_t has them in their positions j and zeros elsewhere."""
    pos, mask = positions(keep, T)
    y = np.zeros(T, np.int64)
    for j in range(n):
        kept = (mask >> j) & 1
        at = start + pos[:T] + POP[mask & ((1 << j) - 1)]
        y |= (kept * bits[np.where(kept == 1, at, 0)].astype(np.int64)) << j
    return y, mask


def step(tr, D, y, k):
    """One step on D [..., S] with received words y and masks k [...]: (D', decisions)."""
    y, k = np.asarray(y)[..., None], np.asarray(k)[..., None]
    c0 = D[..., tr.ps[0]] + POP[(tr.o[0] ^ y) & k]
    c1 = D[..., tr.ps[1]] + POP[(tr.o[1] ^ y) & k]
    dec = c1 < c0                                            # ties keep b = 0
    Dn = np.where(dec, c1, c0)
    return Dn - Dn.min(axis=-1, keepdims=True), dec


def forward(tr, y, mask):
    T = len(y)
    Dall = np.zeros((T + 1, tr.S), np.int64)
    dec = np.zeros((T, tr.S), np.int64)
    for t in range(T):
        Dall[t + 1], dec[t] = step(tr, Dall[t], y[t], mask[t])
    assert Dall.max() <= tr.n * tr.m                         # relative metrics still fit a byte
    return Dall, dec


def traceback(tr, y, mask, Dall, dec, T):
    sT = int(np.argmax(Dall[T] == 0))                        # the lowest-index state with D_T = 0
    s, errors = sT, 0
    bits = np.zeros(T, np.uint8)
    for t in range(T - 1, -1, -1):
        u = s & 1
        prev = (s >> 1) | (int(dec[t, s]) << (tr.m - 1))
        bits[t] = u
        errors += int(POP[(tr.out[prev, u] ^ y[t]) & mask[t]])   # over transmitted bits only
        s = prev
    return bits, errors, s, sT


def counters(tr, y, mask, Dall, dec, T, L, W, Dp):
    """(blocks, forward reruns, traceback fix-ups): cvd_viterbi_decode's definitions."""
    nb = (T + L - 1) // L
    b = np.arange(1, nb)
    reruns = 0
    if len(b):
        Dw = np.zeros((len(b), tr.S), np.int64)
        for j in range(W):
            t = b * L - W + j
            live = t >= 0
            if not live.any():
                continue
            tt = np.maximum(t, 0)
            Dn, _ = step(tr, Dw, y[tt], mask[tt])
            Dw = np.where(live[:, None], Dn, Dw)
        reruns = int((Dw != Dall[b * L]).any(axis=1).sum())
    bb = np.arange(nb)
    e = np.minimum(T, (bb + 1) * L + Dp)
    look = bb[e < T]
    fixups = 0
    if len(look):
        s = np.broadcast_to(np.arange(tr.S), (len(look), tr.S)).copy()
        for j in range(Dp):
            t = (look + 1) * L + Dp - 1 - j
            s = (s >> 1) | (dec[t[:, None], s] << (tr.m - 1))
        fixups = int((s != s[:, :1]).any(axis=1).sum())
    return nb, reruns, fixups


def restatement(tr, bits, keep, start, T, L, W, Dp, fwd=None):
    y, mask = symbols(bits, tr.n, keep, start, T)
    Dall, dec = fwd if fwd is not None else forward(tr, y, mask)
    ub, errors, s0, sT = traceback(tr, y, mask, Dall, dec, T)
    nb, reruns, fixups = counters(tr, y, mask, Dall, dec, T, L, W, Dp)
    span = int(positions(keep, T)[0][T])
    return {"bits": ub, "T": T, "errors": errors, "ber": errors / span, "start_state": s0, "end_state": sT,
            "blocks": nb, "forward_reruns": reruns, "trace_fixups": fixups, "block": L, "warm": W, "depth": Dp,
            "capture_bits": span}


# ───────────────────────────── oracle streams ───────────────────────────────

_CACHE = {}


def code_of(pkg, name):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    k, n, m, gen, _ = cli.code_of(CASES[name][0])
    assert k == 1
    return n, m, gen, pkg.puncture_pattern(CASES[name][1], n)


def punctured_case(pkg, name, p):
    """(trellis, gen, keep, capture bits, forward pass of the TMAX steps from bit JUNK): JUNK
    random bits, the kept bits of the oracle's stream 0 of the code at (TMAX, p), 3 more random
    bits.  Built once per (case, p) and not changed."""
    key = (name, p)
    if key not in _CACHE:
        n, m, gen, keep = code_of(pkg, name)
        words = C.stream(C.Code(gen, m, 1, n), TMAX, p, SEED, C.lib().oc_grid_tag(TMAX, p), 0)
        sent = serial_bits(np.stack([words], axis=1), n).reshape(TMAX, n)
        _, mask = positions(keep, TMAX)
        kept = sent[((mask[:, None] >> np.arange(n)) & 1) == 1]          # row-major: step by step, j ascending
        assert len(kept) == pkg.punctured_bits(TMAX, keep) == positions(keep, TMAX)[0][TMAX]
        rng = np.random.default_rng(11)
        bits = np.concatenate([rng.integers(0, 2, JUNK).astype(np.uint8), kept,
                               rng.integers(0, 2, 3).astype(np.uint8)])
        tr = Trellis(gen, n, m)
        fwd = forward(tr, *symbols(bits, n, keep, JUNK, TMAX))
        for a in fwd:
            a.setflags(write=False)
        _CACHE[key] = (tr, gen, keep, bits, fwd)
    return _CACHE[key]


SHAPES = [
    # T, block, warm, depth
    (1, 32, 64, 40),
    (2, 32, 64, 40),               # T < period (but for m2's period of 2)
    (31, 32, 64, 40),
    (200, 256, 64, 40),
    (768, 256, 64, 40),
    (1297, 256, 100, 40),          # the tail ends inside a period
    (4817, 32, 64, 40),            # blocks and warm-ups start in every column
    (50, 32, 100, 40),             # T < W
    (1100, 1056, 64, 8),           # a segment boundary at step 1,024, mid-period
]


@pytest.mark.parametrize("p", [0.0, 0.05])
@pytest.mark.parametrize("name", sorted(CASES))
def test_decode_equals_restatement(pkg, name, p):
    tr, gen, keep, bits, fwd = punctured_case(pkg, name, p)
    fmt = CASES[name][2]
    rng = np.random.default_rng(3)
    raw = raw_capture(bits, fmt, rng)                    # every bit past the capture is a one
    assert np.array_equal(capture_bits(raw, fmt, len(bits)), bits)
    cap = torch.from_numpy(raw).cuda()
    for T, L, W, Dp in SHAPES:
        want = restatement(tr, bits, keep, JUNK, T, L, W, Dp, fwd=(fwd[0][:T + 1], fwd[1][:T]))
        res = pkg.decode_capture_punctured(tr.n, tr.m, gen, keep, cap, start=JUNK, T=T, format=fmt, nbits=len(bits),
                                           block=L, warm=W, depth=Dp)
        check(res, want)
    # the last kept bit is the capture's last bit (every bit behind it a one): T fits, T + 1 does not
    nbits = JUNK + pkg.punctured_bits(TMAX, keep)
    exact = raw_capture(bits[:nbits], fmt, rng)
    want = restatement(tr, bits, keep, JUNK, TMAX, 256, 64, 40, fwd=fwd)
    check(pkg.decode_capture_punctured(tr.n, tr.m, gen, keep, exact, start=JUNK, T=TMAX, format=fmt, nbits=nbits,
                                       block=256, warm=64, depth=40), want)
    with pytest.raises(pkg.CvdError, match="viterbi_decode_punctured"):
        pkg.decode_capture_punctured(tr.n, tr.m, gen, keep, exact, start=JUNK, T=TMAX + 1, format=fmt, nbits=nbits,
                                     block=256, warm=64, depth=40)
    # the other two formats, and T=None: as many steps as fit in front of the 3 tail bits' end
    T_all = TMAX
    while pkg.punctured_bits(T_all + 1, keep) <= len(bits) - JUNK:
        T_all += 1
    assert T_all > TMAX
    want = restatement(tr, bits, keep, JUNK, T_all, 256, 64, 40)
    for other in sorted({"bytes", "lsb", "msb"} - {fmt}):
        res = pkg.decode_capture_punctured(tr.n, tr.m, gen, keep, raw_capture(bits, other, rng), start=JUNK,
                                           format=other, nbits=len(bits), block=256, warm=64, depth=40)
        check(res, want)


@pytest.mark.parametrize("name", ["m6", "m8"])
def test_all_ones_pattern_is_the_unpunctured_decoder(pkg, name):
    """Nothing erased, at any period: cvd_viterbi_decode's bits and stats[0..8], at an explicit
    setting with reruns and fix-ups and at the defaults (which are then the unpunctured ones)."""
    tr, gen, bits, _ = unpunctured_case(pkg, name, 0.05)
    for setting in (dict(block=32, warm=24, depth=12), dict()):
        base = pkg.decode_capture(tr.n, tr.m, gen, bits, start=JUNK, T=TMAX, **setting)
        if setting:
            assert base["forward_reruns"] > 0 and base["trace_fixups"] > 0
        for period in (1, 3, 16):
            res = pkg.decode_capture_punctured(tr.n, tr.m, gen, [(1 << tr.n) - 1] * period, bits, start=JUNK, T=TMAX,
                                               **setting)
            assert res.pop("capture_bits") == tr.n * TMAX
            assert torch.equal(res["bits"], base["bits"])
            assert {k: v for k, v in res.items() if k != "bits"} == {k: v for k, v in base.items() if k != "bits"}


def test_both_fallback_paths_run_and_stay_exact(pkg):
    """(171,133) at 3/4, L = 32: without warm-up and lookahead every join and lookahead that
    the restatement says fails is counted; a middle setting has some, not all; a generous one
    none; the three results are the same."""
    tr, gen, keep, bits, fwd = punctured_case(pkg, "m6_34", 0.05)
    T, L = TMAX, 32
    got = []
    for W, Dp in ((0, 0), (64, 40), (1536, 512)):
        want = restatement(tr, bits, keep, JUNK, T, L, W, Dp, fwd=fwd)
        print(f"warm {W} depth {Dp}: {want['forward_reruns']} reruns, {want['trace_fixups']} fix-ups "
              f"of {want['blocks']} blocks")
        if (W, Dp) == (0, 0):
            assert want["forward_reruns"] > 0 and want["trace_fixups"] > 0
        elif (W, Dp) == (64, 40):
            assert 0 < want["forward_reruns"] < want["blocks"] - 1
            assert 0 < want["trace_fixups"] < want["blocks"] - 1
        else:
            assert want["forward_reruns"] == 0 and want["trace_fixups"] == 0
        res = pkg.decode_capture_punctured(2, 6, gen, keep, bits, start=JUNK, T=T, block=L, warm=W, depth=Dp)
        check(res, want)
        got.append(res)
    for r in got[1:]:
        assert torch.equal(r["bits"], got[0]["bits"]) and r["errors"] == got[0]["errors"]


def test_survivors_that_never_merge(pkg):
    """(7,5) at 10/11 without noise: most lookaheads fail even at depth 512, so the fix path
    carries nearly every block; the result is the restatement's and the (0, 0) call's."""
    tr, gen, keep, bits, fwd = punctured_case(pkg, "m2", 0.0)
    T, L = TMAX, 32
    deep = restatement(tr, bits, keep, JUNK, T, L, 64, 512, fwd=fwd)
    print(f"depth 512: {deep['trace_fixups']} fix-ups of {deep['blocks']} blocks")
    assert deep["trace_fixups"] > deep["blocks"] // 2
    res = pkg.decode_capture_punctured(2, 2, gen, keep, bits, start=JUNK, T=T, block=L, warm=64, depth=512)
    check(res, deep)
    res0 = pkg.decode_capture_punctured(2, 2, gen, keep, bits, start=JUNK, T=T, block=L, warm=0, depth=0)
    check(res0, restatement(tr, bits, keep, JUNK, T, L, 0, 0, fwd=fwd))
    assert torch.equal(res["bits"], res0["bits"]) and res["errors"] == res0["errors"]


@pytest.mark.parametrize("value", [0, 1])
def test_constant_capture(pkg, value):
    """Tie-heavy: the tie rule with erased bits, and survivors that do not merge."""
    n, m, gen, keep = code_of(pkg, "m6_78")
    tr = Trellis(gen, n, m)
    T, start = 1000, 5
    bits = np.full(start + pkg.punctured_bits(T, keep) + 1, value, np.uint8)
    for L, W, Dp in ((32, 64, 40), (256, 0, 0)):
        want = restatement(tr, bits, keep, start, T, L, W, Dp)
        check(pkg.decode_capture_punctured(n, m, gen, keep, bits, start=start, T=T, block=L, warm=W, depth=Dp), want)


def test_bit_positions_past_2_31(pkg):
    """A packed random capture of 2^31 + 2^20 bits (256 MiB): steps whose bits lie past bit
    2^31 against the restatement on those bytes."""
    n, m, gen, keep = code_of(pkg, "m6_34")
    tr = Trellis(gen, n, m)
    nbits = (1 << 31) + (1 << 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    cap = torch.randint(0, 256, (nbits // 8,), dtype=torch.uint8, device="cuda", generator=g)
    start, T = (1 << 31) + 12345, 2001
    tail = np.unpackbits(cap[start // 8:(start + n * T) // 8 + 1].cpu().numpy(), bitorder="little")
    want = restatement(tr, tail, keep, start % 8, T, 256, 64, 40)
    check(pkg.decode_capture_punctured(n, m, gen, keep, cap, start=start, T=T, format="lsb", nbits=nbits, block=256,
                                       warm=64, depth=40), want)


def mid_period_capture(pkg):
    """The noiseless (171,133) 3/4 stream cut so that it begins with step 1: the next period
    begins 2 bits (steps 1 and 2, one bit each) behind the JUNK prefix."""
    tr, gen, keep, bits, _ = punctured_case(pkg, "m6_34", 0.0)
    assert keep == [3, 2, 1]
    return tr, gen, keep, np.concatenate([bits[:JUNK], bits[JUNK + 2:]]), 2


def test_sync_punctured(pkg):
    tr, gen, keep, bits, true_offset = mid_period_capture(pkg)
    dec = importlib.import_module(pkg.__name__ + ".decode")
    T, K = 1000, 4
    W, Dp = dec.default_warm_punctured(6, 2, 3, K), dec.default_depth_punctured(6, 2, 3, K)
    want = []
    for o in range(K):
        r = restatement(tr, bits, keep, JUNK + o, T, 4096, W, Dp)
        r["offset"] = o
        want.append(r)
    want.sort(key=lambda r: (r["errors"], r["offset"]))
    assert want[0]["offset"] == true_offset and want[0]["errors"] == 0 and want[1]["errors"] > 0
    got = pkg.sync_punctured(2, 6, gen, keep, bits, start=JUNK, T=T)
    assert len(got) == K
    for g, w in zip(got, want):
        check(g, w)                                      # the resolved defaults among the rest


def test_decode_cli_punctured(pkg, tmp_path, capsys):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    tr, gen, keep, bits, true_offset = mid_period_capture(pkg)
    npy, out = str(tmp_path / "capture.npy"), str(tmp_path / "res")
    np.save(npy, bits)
    assert cli.main(["decode", "--code", "oct:171,133", "--input", npy, "--start", str(JUNK), "--puncture", "dvb:3/4",
                     "--sync", "1000", "--save-dir", out]) == 0
    offset = pkg.sync_punctured(2, 6, gen, keep, bits, start=JUNK, T=1000)[0]["offset"]
    assert offset == true_offset
    want = pkg.decode_capture_punctured(2, 6, gen, keep, bits, start=JUNK + offset)
    want["offset"] = offset
    got = np.load(str(tmp_path / "res" / "decoded.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, want["bits"].cpu().numpy())
    with open(str(tmp_path / "res" / "decode.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == cli.DECODE_COLUMNS + ["capture_bits", "offset"]
    assert len(rows) == 2
    assert [float(v) if c == "ber" else int(v) for c, v in zip(rows[0], rows[1])] == [want[c] for c in rows[0]]
    assert want["T"] >= TMAX - 3 and want["errors"] == 0 and want["offset"] == 2
    printed = capsys.readouterr().out
    assert re.search(r"p = (\S+) ", printed).group(1) == repr(want["ber"])
    assert "scan --code" not in printed

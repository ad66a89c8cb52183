"""Soft-decision decoding of a capture on the GPU: cvd_viterbi_decode_soft against a numpy
restatement of the header (test_gpu_decode.py's sequential decoder and counter definitions with
the soft cost in the place of the popcount), on the C oracle's streams given seeded magnitudes,
erasures and -128s behind a junk prefix; against the hard decoder on +-A captures and against
the punctured decoder on depunctured ones.  Every expected value is exact; no test asserts a
statistical outcome.  The shapes are those of the punctured decoder's tests: T of 1, 2 and 31, a
ragged tail, 150 blocks of 32, T below the warm-up, a segment boundary at step 1,024, 2^m below,
at and above a wavefront's 64 lanes, n = 3, and a capture that begins at an odd byte."""
import csv
import ctypes
import importlib

import numpy as np
import pytest
import torch

from test_gpu_capture import JUNK
from test_gpu_decode import CODES, TMAX, Trellis, check, counters, oracle_case
from test_gpu_decode_punctured import SHAPES, mid_period_capture, positions, punctured_case

pytestmark = pytest.mark.gpu


# ───────────────────────────── numpy restatement ────────────────────────────

def cost(o, v):
    """cost(out, t) of include/cvd.h for the outputs o [S] and the values v [..., n] -> [..., S]."""
    v = np.asarray(v, np.int64)
    v = np.maximum(v, -127)[..., None]                           # -128 is read as -127
    c = 0
    for j in range(v.shape[-2]):
        bit = ((o >> j) & 1) == 1
        c = c + np.abs(v[..., j, :]) * ((v[..., j, :] != 0) & ((v[..., j, :] > 0) != bit))
    return c


class SoftTrellis(Trellis):
    def step(self, D, v):
        """test_gpu_decode.py's step on D [..., S] with the values v [..., n] of the step."""
        c0 = D[..., self.ps[0]] + cost(self.o[0], v)
        c1 = D[..., self.ps[1]] + cost(self.o[1], v)
        dec = c1 < c0                                            # ties keep b = 0
        Dn = np.where(dec, c1, c0)
        return Dn - Dn.min(axis=-1, keepdims=True), dec


def values(soft, n, start, T):
    return np.asarray(soft[start:start + n * T], np.int64).reshape(T, n)


def forward(tr, v):
    T = len(v)
    Dall = np.zeros((T + 1, tr.S), np.int64)
    dec = np.zeros((T, tr.S), np.int64)
    for t in range(T):
        Dall[t + 1], dec[t] = tr.step(Dall[t], v[t])
    assert Dall.max() <= 127 * tr.n * tr.m                       # relative metrics fit 16 bits
    return Dall, dec


def traceback(tr, v, Dall, dec, T):
    sT = int(np.argmax(Dall[T] == 0))                            # the lowest-index state with D_T = 0
    s, metric, errors = sT, 0, 0
    bits = np.zeros(T, np.uint8)
    for t in range(T - 1, -1, -1):
        u = s & 1
        prev = (s >> 1) | (int(dec[t, s]) << (tr.m - 1))
        bits[t] = u
        out = np.array([tr.out[prev, u]])
        metric += int(cost(out, v[t])[0])
        errors += int(cost(out, np.sign(v[t]))[0])
        s = prev
    return bits, metric, errors, s, sT


def restatement(tr, soft, start, T, L, W, Dp, fwd=None):
    v = values(soft, tr.n, start, T)
    Dall, dec = fwd if fwd is not None else forward(tr, v)
    ub, metric, errors, s0, sT = traceback(tr, v, Dall, dec, T)
    nb, reruns, fixups = counters(tr, v, Dall, dec, T, L, W, Dp)
    seen = int((v != 0).sum())
    return {"bits": ub, "T": T, "errors": errors, "ber": errors / seen if seen else 0.0, "start_state": s0,
            "end_state": sT, "blocks": nb, "forward_reruns": reruns, "trace_fixups": fixups, "block": L, "warm": W,
            "depth": Dp, "metric": metric, "erasures": tr.n * T - seen}


# ───────────────────────────── soft captures ────────────────────────────────

_CACHE = {}


def soft_case(pkg, name):
    """(trellis, gen, soft capture, forward pass of the TMAX steps from value JUNK): the bits of
    oracle_case(name, 0.05) with seeded magnitudes in 1..127, one value in eight erased, one in
    thirty -128, and the first value behind the junk -128.  Built once per code, not changed."""
    if name not in _CACHE:
        htr, gen, bits, _ = oracle_case(pkg, name, 0.05)
        rng = np.random.default_rng(17)
        soft = (2 * bits.astype(np.int64) - 1) * rng.integers(1, 128, len(bits))
        soft[rng.random(len(bits)) < 1 / 8] = 0
        soft[rng.random(len(bits)) < 1 / 30] = -128
        soft[JUNK] = -128
        soft = soft.astype(np.int8)
        tr = SoftTrellis(gen, htr.n, htr.m)
        fwd = forward(tr, values(soft, tr.n, JUNK, TMAX))
        for a in fwd + (soft,):
            a.setflags(write=False)
        _CACHE[name] = (tr, gen, soft, fwd)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_equals_restatement(pkg, name):
    tr, gen, soft, fwd = soft_case(pkg, name)
    assert JUNK % 16 != 0 and soft[JUNK] == -128 and (soft == 0).any() and (soft[JUNK + 1:] == -128).any()
    cap = torch.from_numpy(soft.copy()).cuda()
    for T, L, W, Dp in SHAPES:
        want = restatement(tr, soft, JUNK, T, L, W, Dp, fwd=(fwd[0][:T + 1], fwd[1][:T]))
        check(pkg.decode_capture_soft(tr.n, tr.m, gen, cap, start=JUNK, T=T, block=L, warm=W, depth=Dp), want)
    # the last value is the capture's last: T fits, T + 1 does not
    exact = soft[:JUNK + tr.n * TMAX]
    want = restatement(tr, soft, JUNK, TMAX, 256, 64, 40, fwd=fwd)
    check(pkg.decode_capture_soft(tr.n, tr.m, gen, exact, start=JUNK, T=TMAX, block=256, warm=64, depth=40), want)
    with pytest.raises(pkg.CvdError, match="viterbi_decode_soft"):
        pkg.decode_capture_soft(tr.n, tr.m, gen, exact, start=JUNK, T=TMAX + 1, block=256, warm=64, depth=40)
    # T=None: as many whole steps as fit (the 3 tail values: one more step for n = 2, 3)
    T_all = (len(soft) - JUNK) // tr.n
    assert T_all == TMAX + 1
    check(pkg.decode_capture_soft(tr.n, tr.m, gen, soft, start=JUNK, block=256, warm=64, depth=40),
          restatement(tr, soft, JUNK, T_all, 256, 64, 40))


@pytest.mark.parametrize("name", ["m6", "m8"])
def test_constant_magnitude_is_the_hard_decoder(pkg, name):
    """Every value +-A: the hard decoder's bits, states and counters, at an explicit setting with
    reruns and fix-ups and at the defaults; the soft distance is A times the error count."""
    tr, gen, bits, _ = oracle_case(pkg, name, 0.05)
    for setting in (dict(block=32, warm=24, depth=12), dict()):
        base = pkg.decode_capture(tr.n, tr.m, gen, bits, start=JUNK, T=TMAX, **setting)
        if setting:
            assert base["forward_reruns"] > 0 and base["trace_fixups"] > 0
        for A in (1, 127):
            res = pkg.decode_capture_soft(tr.n, tr.m, gen, pkg.soft_from_bits(bits, A), start=JUNK, T=TMAX, **setting)
            assert res.pop("metric") == A * base["errors"]
            assert res.pop("erasures") == 0
            assert torch.equal(res["bits"], base["bits"])
            assert {k: v for k, v in res.items() if k != "bits"} == {k: v for k, v in base.items() if k != "bits"}


@pytest.mark.parametrize("name", ["m6_34", "m6_78", "m3n3"])
def test_depunctured_is_the_punctured_decoder(pkg, name):
    """+-1 at the kept positions and zeros at the erased ones: cvd_viterbi_decode_punctured's
    bits, states and counters at equal block, warm and depth, and at the defaults."""
    tr, gen, keep, bits, _ = punctured_case(pkg, name, 0.05)
    soft = pkg.soft_from_bits(bits)
    for setting in (dict(block=32, warm=24, depth=12), dict()):
        base = pkg.decode_capture_punctured(tr.n, tr.m, gen, keep, bits, start=JUNK, T=TMAX, **setting)
        res = pkg.decode_capture_soft(tr.n, tr.m, gen, soft, start=JUNK, T=TMAX, keep=keep, **setting)
        assert res.pop("metric") == base["errors"]
        assert res.pop("erasures") == tr.n * TMAX - base["capture_bits"]
        assert torch.equal(res["bits"], base["bits"])
        assert {k: v for k, v in res.items() if k != "bits"} == {k: v for k, v in base.items() if k != "bits"}
    # T=None: as many steps as fit, as there
    base = pkg.decode_capture_punctured(tr.n, tr.m, gen, keep, bits, start=JUNK)
    res = pkg.decode_capture_soft(tr.n, tr.m, gen, soft, start=JUNK, keep=keep)
    assert res["T"] == base["T"] > TMAX and res["capture_bits"] == base["capture_bits"]
    assert torch.equal(res["bits"], base["bits"]) and res["errors"] == res["metric"] == base["errors"]


def depunctured(soft, n, keep, start, T):
    """cvd_soft_depuncture in numpy."""
    pos, mask = positions(keep, T)
    out = np.zeros((T, n), np.int8)
    rank = np.zeros(T, np.int64)
    for j in range(n):
        kept = ((mask >> j) & 1) == 1
        out[kept, j] = soft[start + pos[:T][kept] + rank[kept]]
        rank += kept
    return out.reshape(-1)


@pytest.mark.parametrize("n,keep,T", [(2, [3, 2, 1], 1297), (3, [7, 1, 6, 2, 5], 1298), (2, [3, 2, 2, 2, 1, 2, 1], 3),
                                      (3, [7], 16), (2, [1, 3], 1)])
def test_soft_depuncture(pkg, n, keep, T):
    """cvd_soft_depuncture alone: a tail that ends inside a period, n T that is and is not a
    multiple of 16, zero padding up to 16 bytes and nothing written behind it."""
    span = pkg.punctured_bits(T, keep)
    rng = np.random.default_rng(23)
    soft = rng.integers(-128, 128, JUNK + span, dtype=np.int8)
    soft[soft == 0] = 1                                          # zeros in the output are erasures only
    want = depunctured(soft, n, keep, JUNK, T)
    assert (T % len(keep) != 0 or len(keep) == 1) and (want == 0).sum() == n * T - span
    padded = (n * T + 15) // 16 * 16
    src = torch.from_numpy(soft).cuda()                          # any alignment, no padding: only values < nvals are read
    dst = torch.full((padded + 16,), 77, dtype=torch.int8, device="cuda")
    rc = pkg.lib().cvd_soft_depuncture(ctypes.c_void_p(src.data_ptr()), len(soft), JUNK, bytes(keep), len(keep), n, T,
                                       ctypes.c_void_p(dst.data_ptr()), None)
    assert rc == 0, pkg.lib().cvd_last_error()
    got = dst.cpu().numpy()
    assert np.array_equal(got[:n * T], want)
    assert not got[n * T:padded].any() and (got[padded:] == 77).all()
    assert np.array_equal(pkg.depuncture_soft(soft, keep, n, start=JUNK, T=T).cpu().numpy(), want)
    assert np.array_equal(pkg.depuncture_soft(soft, keep, n, start=JUNK).cpu().numpy(), want)   # T=None: what fits


def test_both_fallback_paths_run_and_stay_exact(pkg):
    """L = 32 without warm-up and lookahead: an all-zero warm vector is almost never the true
    one and no lookahead of depth 0 certifies, so nearly every block is rerun and fixed; a
    generous setting has none; the results are the same."""
    tr, gen, soft, fwd = soft_case(pkg, "m6")
    T, L = TMAX, 32
    none = restatement(tr, soft, JUNK, T, L, 0, 0, fwd=fwd)
    nb = none["blocks"]
    print(f"warm 0 depth 0: {none['forward_reruns']} reruns, {none['trace_fixups']} fix-ups of {nb} blocks")
    assert none["forward_reruns"] >= nb - 3 and none["trace_fixups"] == nb - 1
    res0 = pkg.decode_capture_soft(2, 6, gen, soft, start=JUNK, T=T, block=L, warm=0, depth=0)
    check(res0, none)
    generous = restatement(tr, soft, JUNK, T, L, 1536, 512, fwd=fwd)
    assert generous["forward_reruns"] == 0 and generous["trace_fixups"] == 0
    res1 = pkg.decode_capture_soft(2, 6, gen, soft, start=JUNK, T=T, block=L, warm=1536, depth=512)
    check(res1, generous)
    assert torch.equal(res0["bits"], res1["bits"]) and res0["metric"] == res1["metric"]


@pytest.mark.parametrize("value", [127, 0])
def test_constant_capture(pkg, value):
    """n = 3, m = 8.  All +127: tie-heavy, and the relative metrics go to the bound.  All zero:
    every value an erasure, every decision a tie."""
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    k, n, m, gen, _ = cli.code_of("oct:557,663,711")
    assert (k, n, m) == (1, 3, 8)
    tr = SoftTrellis(gen, n, m)
    T, start = 1000, 5
    soft = np.full(start + n * T + 1, value, np.int8)
    for L, W, Dp in ((32, 64, 40), (256, 0, 0)):
        want = restatement(tr, soft, start, T, L, W, Dp)
        if value == 0:
            assert want["metric"] == 0 and want["ber"] == 0.0 and want["erasures"] == n * T and want["errors"] == 0
        check(pkg.decode_capture_soft(n, m, gen, soft, start=start, T=T, block=L, warm=W, depth=Dp), want)


def test_value_positions_past_2_31(pkg):
    """A device-generated capture of 2^31 + 2^20 values (2 GiB): steps whose values lie past
    index 2^31 against the restatement on that slice."""
    tr, gen, _, _ = soft_case(pkg, "m6")
    nvals = (1 << 31) + (1 << 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    cap = torch.randint(-128, 128, (nvals,), dtype=torch.int8, device="cuda", generator=g)
    start, T = (1 << 31) + 12345, 2001
    tail = cap[start:start + tr.n * T].cpu().numpy()
    want = restatement(tr, tail, 0, T, 256, 64, 40)
    check(pkg.decode_capture_soft(tr.n, tr.m, gen, cap, start=start, T=T, block=256, warm=64, depth=40), want)


def test_sync_punctured_soft(pkg):
    """On a +-A capture the soft distance is A times the error count: sync_punctured's ranking."""
    tr, gen, keep, bits, true_offset = mid_period_capture(pkg)
    want = pkg.sync_punctured(2, 6, gen, keep, bits, start=JUNK, T=1000)
    got = pkg.sync_punctured_soft(2, 6, gen, keep, pkg.soft_from_bits(bits, 9), start=JUNK, T=1000)
    assert [r["offset"] for r in got] == [r["offset"] for r in want] and got[0]["offset"] == true_offset
    for g, w in zip(got, want):
        assert g["metric"] == 9 * w["errors"] and g["errors"] == w["errors"]
        assert torch.equal(g["bits"], w["bits"]) and g["capture_bits"] == w["capture_bits"]


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert len(rows) == 2
    return rows[0], [float(v) if c == "ber" else int(v) for c, v in zip(rows[0], rows[1])]


def test_decode_cli_soft(pkg, tmp_path, capsys):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    tr, gen, soft, _ = soft_case(pkg, "m6")
    npy, out = str(tmp_path / "soft.npy"), str(tmp_path / "res")
    np.save(npy, soft)
    assert cli.main(["decode", "--code", CODES["m6"][0], "--input", npy, "--format", "soft", "--start", str(JUNK),
                     "--save-dir", out]) == 0
    want = pkg.decode_capture_soft(2, 6, gen, soft, start=JUNK)
    assert want["T"] == TMAX + 1 and want["erasures"] > 0 and want["metric"] > 0
    got = np.load(str(tmp_path / "res" / "decoded.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, want["bits"].cpu().numpy())
    columns, row = read_csv(str(tmp_path / "res" / "decode.csv"))
    assert columns == cli.DECODE_COLUMNS + ["metric", "erasures"]
    assert row == [want[c] for c in columns]
    printed = capsys.readouterr().out
    assert "scan --code" not in printed
    # --nbits counts values: one step less fits
    assert cli.main(["decode", "--code", CODES["m6"][0], "--input", npy, "--format", "soft", "--start", str(JUNK),
                     "--nbits", str(len(soft) - 2), "--save-dir", out]) == 0
    assert read_csv(str(tmp_path / "res" / "decode.csv"))[1][0] == TMAX
    capsys.readouterr()


def test_decode_cli_soft_punctured(pkg, tmp_path, capsys):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    tr, gen, keep, bits, true_offset = mid_period_capture(pkg)
    soft = pkg.soft_from_bits(bits, 50)
    raw, out = str(tmp_path / "soft.bin"), str(tmp_path / "res")
    soft.tofile(raw)                                     # a raw file is read as int8
    assert cli.main(["decode", "--code", "oct:171,133", "--input", raw, "--format", "soft", "--start", str(JUNK),
                     "--puncture", "dvb:3/4", "--sync", "1000", "--save-dir", out]) == 0
    offset = pkg.sync_punctured_soft(2, 6, gen, keep, soft, start=JUNK, T=1000)[0]["offset"]
    assert offset == true_offset == 2
    want = pkg.decode_capture_soft(2, 6, gen, soft, start=JUNK + offset, keep=keep)
    want["offset"] = offset
    got = np.load(str(tmp_path / "res" / "decoded.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, want["bits"].cpu().numpy())
    columns, row = read_csv(str(tmp_path / "res" / "decode.csv"))
    assert columns == cli.DECODE_COLUMNS + ["metric", "erasures", "capture_bits", "offset"]
    assert row == [want[c] for c in columns]
    assert want["T"] >= TMAX - 3 and want["errors"] == 0 and want["metric"] == 0
    assert want["erasures"] == 2 * want["T"] - want["capture_bits"]
    assert "scan --code" not in capsys.readouterr().out

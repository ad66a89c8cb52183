"""The bit-sliced BSC generator (csrc/cvd_kernels.hip: noise_planes4, noise_head,
noise_head_planes, noise_exchange_pair / _split, noise_chunk_wave, ChunkEncoder::chunk / head /
finish; gen_fast_kernel's fast and small forms, the fused trial kernel) at every plane depth and
threshold edge, against the oracle.  A code bit is still undecided after n planes with
probability 2^-n whatever p is, so random streams reach the straggler rounds past plane 16 a
few hundred times and plane 25 almost never; here the threshold is put where a chosen bit is
decided exactly at plane d, for every d, or is equal through all 32 (tests/noise_cases.py; the
cases themselves are checked on the CPU in test_noise_cases_host.py).  The fused kernel's tag
is tied to p, so its deep planes come from a committed search instead.  Every comparison is
exact."""
import contextlib
import os
import time

import numpy as np
import pytest
import torch

import noise_cases as NC
from conftest import code_of
from oracle import c_oracle as C
from oracle import philox
from oracle import restatement as R
from test_gpu_learn import _pair
from test_gpu_parity import unpack_words

pytestmark = pytest.mark.gpu

K1N3 = [[[1, 0, 1, 1, 1]], [[1, 1, 0, 1, 1]], [[1, 1, 1, 1, 1]]]           # test_gpu_parity.py's k1n3
GEN_ENV = ("CVD_GEN_FORM", "CVD_GEN_TAP_LOOP", "CVD_GEN_GENERIC", "CVD_GEN_SLOTS")
CODE_NAMES = ["m6", "k1n3", "r23_m4"]


def _variants(n, generic=True):
    """generator variants: (label, environment)"""
    v = [("fast", {"CVD_GEN_FORM": "fast"}), ("small", {"CVD_GEN_FORM": "small"})] if n == 2 else [("default", {})]
    v.append(("tap_loop", {"CVD_GEN_TAP_LOOP": "1"}))
    if generic:
        v.append(("generic", {"CVD_GEN_GENERIC": "1"}))
    return v


@contextlib.contextmanager
def _env(monkeypatch, env):
    old = {key: os.environ.get(key) for key in env}
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    try:
        yield
    finally:
        for key, val in old.items():
            if val is None:
                monkeypatch.delenv(key)
            else:
                monkeypatch.setenv(key, val)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for key in GEN_ENV:
        monkeypatch.delenv(key, raising=False)


@pytest.fixture(scope="module")
def codes(pkg, golden):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    out = {}
    for name in CODE_NAMES:
        if name == "m6":
            k, n, m, taps = 1, 2, 6, pkg.CONFIG_CODES["m6"]["gen1"]
        elif name == "k1n3":
            k, n, m, taps = 1, 3, 4, K1N3
        else:
            k, n, m, taps = code_of(golden[1], "r23_m4")
        out[name] = (k, n, m, taps, pkg.Detector(k, n, m, taps, device=0), C.Code(taps, m, k, n))
    return out


def _launch_all(det, taps, N, thrs, base, variants, monkeypatch):
    """{label: [len(thrs), W/4, COUNT, 4]}: all thresholds of one variant back to back"""
    out = {}
    for label, env in variants:
        with _env(monkeypatch, env):
            out[label] = torch.stack([det.generate(taps, N, NC.p_of(thr), NC.SEED, NC.TAG, base, NC.STRIDE, NC.COUNT)
                                      for thr in thrs])
    torch.cuda.synchronize()
    return out


def _oracle_words(code, N, p, base):
    """[N, COUNT] received words of the launch's sequences (C oracle)"""
    return np.stack([C.stream(code, N, p, NC.SEED, NC.TAG, NC.seq_of(q, base)) for q in range(NC.COUNT)], axis=1)


def _check_padding(buf, n, N):
    """words past the last live one, and the last word's bits past step N, stay zero"""
    spw = 32 // n
    nwords = -(-N // spw)
    last = buf[-1].cpu().numpy().view(np.uint32)                  # [COUNT, 4]: the last chunk
    live = nwords - 4 * (buf.shape[0] - 1)
    assert 1 <= live <= 4
    if live < 4:
        assert int(last[:, live:].max()) == 0
    rem = (N - (nwords - 1) * spw) * n
    if rem < 32:
        assert int((last[:, live - 1] >> rem).max()) == 0


def _check_target(codes, name, N, base, target, cases, variants, monkeypatch, ref_variants=None):
    """One target bit under `cases` [(label, thr, flips)]: all variants equal, all sequences equal
    the C oracle, the target sequence equals the numpy restatement, the target bit does as
    predicted.  ref_variants: compared too, launched without the caller's environment."""
    k, n, m, taps, det, code = codes[name]
    q, w, b = target
    sid = NC.seq_of(q, base)
    spw = 32 // n
    t, j = w * spw + b // n, b % n
    u = NC.uniform_of(NC.SEED, NC.TAG, sid, w, b)
    thrs = [thr for _, thr, _ in cases(u)]
    got = _launch_all(det, taps, N, thrs, base, variants, monkeypatch)
    first = got[variants[0][0]]
    for label, _ in variants[1:]:
        assert torch.equal(first, got[label]), (name, target, label)
    if ref_variants is not None:
        assert torch.equal(first, ref_variants(thrs)), (name, target, "reference launch")
    clean = C.stream(code, N, 0.0, NC.SEED, NC.TAG, sid)
    first = first.cpu()
    for i, (label, thr, flips) in enumerate(cases(u)):
        p = NC.p_of(thr)
        words = unpack_words(first[i], n, N)
        np.testing.assert_array_equal(words, _oracle_words(code, N, p, base), err_msg=f"{name} {target} {label}")
        np.testing.assert_array_equal(words[:, q], R.received_stream(taps, m, k, n, N, p, NC.SEED, NC.TAG, sid))
        assert ((int(words[t, q]) ^ int(clean[t])) >> j) & 1 == flips, (name, target, label, hex(u), hex(thr))
        _check_padding(first[i], n, N)
    return len(thrs)


# ─────────────── 3a: every depth, every generator variant ───────────────

@pytest.mark.parametrize("name", CODE_NAMES)
def test_every_depth_every_variant(codes, name, monkeypatch):
    n = codes[name][1]
    for target in NC.TARGETS[n]:
        assert _check_target(codes, name, NC.N_SHORT[n], NC.BASE, target, NC.all_cases, _variants(n), monkeypatch) == 66


@pytest.mark.parametrize("name", CODE_NAMES)
def test_every_depth_sequence_ids_past_32_bits(codes, name, monkeypatch):
    """seq_base = 2^33 + 7: the slot lanes' (seq_lo, ctr_hi) of another lane's sequence, ctr_hi != 0"""
    n = codes[name][1]
    _check_target(codes, name, NC.N_SHORT[n], NC.BASE_HI, NC.TARGET_HI, NC.all_cases, _variants(n), monkeypatch)


def test_every_depth_in_the_last_segment_of_a_split_launch(codes, monkeypatch):
    """N = 4099 (257 words, 65 chunks): gridDim.y = 4 segments, enc.seek runs first; the target is
    the single live word of the last chunk"""
    _check_target(codes, "m6", NC.N_LONG, NC.BASE, NC.TARGET_LONG, NC.all_cases, _variants(2), monkeypatch)


# ─────────────── 3b: the deep rounds in several exchange rounds ───────────────

@pytest.mark.parametrize("slots", ["1", "2", "3"])
@pytest.mark.parametrize("name", CODE_NAMES)
def test_deep_rounds_in_several_exchange_rounds(codes, name, slots, monkeypatch):
    """CVD_GEN_SLOTS = 1, 2, 3 (the split form's npr = 1, the pair form's single slot): the same
    buffers as with 64 slots, equal to the oracle"""
    k, n, m, taps, det, code = codes[name]
    variants = _variants(n, generic=False)

    def default_launch(thrs):
        with _env(monkeypatch, {"CVD_GEN_SLOTS": "64"}):
            return _launch_all(det, taps, NC.N_SHORT[n], thrs, NC.BASE, variants[:1], monkeypatch)[variants[0][0]]

    monkeypatch.setenv("CVD_GEN_SLOTS", slots)
    for target in NC.TARGETS[n]:
        _check_target(codes, name, NC.N_SHORT[n], NC.BASE, target, NC.deep_cases, variants, monkeypatch,
                      ref_variants=default_launch)


# ─────────────── 3c: threshold edges ───────────────

@pytest.mark.parametrize("name", CODE_NAMES)
def test_threshold_edges_generator(codes, name, monkeypatch):
    """thr_all, the clamp thr_lo = min(thr, 2^32 - 1), the thr_lo == 0 bypass, single low bits"""
    k, n, m, taps, det, code = codes[name]
    assert [philox.threshold(p) for p in NC.EDGE_P] == NC.EDGE_THR
    N = NC.N_SHORT[n]
    variants = _variants(n)
    got = {}
    for label, env in variants:
        with _env(monkeypatch, env):
            got[label] = [det.generate(taps, N, p, NC.SEED, NC.TAG, NC.BASE, NC.STRIDE, NC.COUNT) for p in NC.EDGE_P]
    torch.cuda.synchronize()
    for i, p in enumerate(NC.EDGE_P):
        first = got[variants[0][0]][i]
        for label, _ in variants[1:]:
            assert torch.equal(first, got[label][i]), (name, p, label)
        np.testing.assert_array_equal(unpack_words(first, n, N), _oracle_words(code, N, p, NC.BASE), err_msg=f"{name} p={p!r}")
        _check_padding(first, n, N)


EDGE_N, EDGE_LO, EDGE_TRIALS, EDGE_SEED = 1237, 3_000_000_011, 1237, 777   # a partial last word for n = 2 and 3


@pytest.mark.parametrize("cfg", ["m2", "r23_m4"])
def test_threshold_edges_fused(pkg, cfg):
    """one model learned at p = 0.05; the trials' p at the edges: fused == two-kernel path == C oracle"""
    cc = pkg.CONFIG_CODES[cfg]
    k, n, m, g1, g2 = cc["k"], cc["n"], cc["m"], cc["gen1"], cc["gen2"]
    assert EDGE_N % (32 // n) != 0
    det = pkg.Detector(k, n, m, g1, device=0)
    model = det.model(0.05, None, 200, 1.0, EDGE_SEED)
    c1, c2 = C.Code(g1, m, k, n), C.Code(g2, m, k, n)
    cm = C.Model(c1, 0.05, None, 200, 1.0, EDGE_SEED)
    lo, hi = EDGE_LO, EDGE_LO + EDGE_TRIALS
    for p in NC.EDGE_P:
        got = det.run_trials(model, g1, g2, EDGE_N, p, EDGE_SEED, lo, hi, return_sums=True, fused=True)
        ref = det.run_trials(model, g1, g2, EDGE_N, p, EDGE_SEED, lo, hi, return_sums=True)
        assert np.array_equal(got["sums"], ref["sums"]), (cfg, p)
        assert got["counts"].cpu().tolist() == ref["counts"].cpu().tolist(), (cfg, p)
        _, want = cm.run_trials(c1, c2, EDGE_N, p, EDGE_SEED, lo, lo + 64, sums=True)
        assert np.array_equal(got["sums"][:64], want), (cfg, p)


def test_threshold_edges_m6_bitsliced(pkg):
    """the default m = 6 path (generator beside the bit-sliced detector) at the edges vs the C oracle"""
    cc = pkg.CONFIG_CODES["m6"]
    det = pkg.Detector(1, 2, 6, cc["gen1"], device=0)
    model = det.model(0.05, 60_000, 200, 1.0, EDGE_SEED)
    c1, c2 = C.Code(cc["gen1"], 6, 1, 2), C.Code(cc["gen2"], 6, 1, 2)
    cm = C.Model(c1, 0.05, 60_000, 200, 1.0, EDGE_SEED)
    for p in NC.EDGE_P:
        got = det.run_trials(model, cc["gen1"], cc["gen2"], EDGE_N, p, EDGE_SEED, EDGE_LO, EDGE_LO + 16, return_sums=True)
        cnt, want = cm.run_trials(c1, c2, EDGE_N, p, EDGE_SEED, EDGE_LO, EDGE_LO + 16, sums=True)
        assert np.array_equal(got["sums"], want), p
        assert tuple(got["counts"].cpu().tolist()) == tuple(int(x) for x in cnt), p
    assert model.device_error() == 0


# ─────────────── 3d: the fused kernel's deep planes, by search ───────────────

@pytest.mark.parametrize("cfg", ["m2", "r23_m4"])
def test_fused_deep_planes_by_search(pkg, cfg, monkeypatch):
    cc = pkg.CONFIG_CODES[cfg]
    k, n, m, g1, g2 = cc["k"], cc["n"], cc["m"], cc["gen1"], cc["gen2"]
    c = NC.FUSED_DEEP[cfg]
    N, p, seed, t0, T = c["N"], c["p"], c["seed"], c["trial_begin"], c["trials"]
    spw = 32 // n
    assert N % spw == 0 and 2 * T * N * n >= 2 ** 27 - 2 * N * n
    # from the oracle alone: at least three bits decided at plane 25 or later, under both hypotheses
    t_start = time.perf_counter()
    hist, deep = NC.depth_histogram(seed, philox.grid_tag(N, p), np.arange(2 * t0, 2 * (t0 + T), dtype=np.uint64),
                                    N // spw, n, philox.threshold(p), deep_from=25)
    t_search = time.perf_counter() - t_start
    assert hist.sum() == 2 * T * N * n and hist[25:].sum() == len(deep) >= 3
    assert any(s % 2 == 0 for s, _, _, _ in deep) and any(s % 2 == 1 for s, _, _, _ in deep)
    print(f"\n  {cfg}: depth histogram {hist[1:].tolist()} ({t_search:.1f} s); deep bits (seq_id, w, b, depth) {deep}; "
          f"deepest {max(d for _, _, _, d in deep)}")
    det = pkg.Detector(k, n, m, g1, device=0)
    model = det.model(p, None, 200, 1.0, seed)
    c1, c2 = C.Code(g1, m, k, n), C.Code(g2, m, k, n)
    cm = C.Model(c1, p, None, 200, 1.0, seed)
    for w0 in sorted({(s // 2) // 64 * 64 for s, _, _, _ in deep}):   # the aligned 64 trial ids around each
        cnt, want = cm.run_trials(c1, c2, N, p, seed, w0, w0 + 64, sums=True)
        for slots in (None, "3", "1"):   # (the pair form's single slot)
            with _env(monkeypatch, {} if slots is None else {"CVD_GEN_SLOTS": slots}):
                got = det.run_trials(model, g1, g2, N, p, seed, w0, w0 + 64, return_sums=True, fused=True)
            assert np.array_equal(got["sums"], want), (cfg, w0, slots)
            assert tuple(got["counts"].cpu().tolist()) == tuple(int(x) for x in cnt), (cfg, w0, slots)


# ─────────────── 3e: the learning chain ───────────────

@pytest.mark.parametrize("case", ["plane32", "equal"])
def test_learning_chain_deep_bit(pkg, case):
    """the learning stream (LEARN_TAG, sequence 0, one live lane) with a bit of its first 60,000
    steps decided at plane 32, or equal through plane 32: host and GPU chains build the same model,
    and for m = 6 the C oracle's (two chains that share a noise bug would still agree)"""
    w, b, u = NC.learn_target()
    thr = NC.crafted(u, 32)[0] if case == "plane32" else NC.crafted_equal(u)[0]
    p = NC.p_of(thr)
    assert 0.01 <= p <= 0.2 and NC.depth_of(u, thr) == (32 if case == "plane32" else 33)
    for cfg in ("m6", "m2"):
        cc = pkg.CONFIG_CODES[cfg]
        host, _ = _pair(pkg, cc["gen1"], cc["m"], cc["k"], cc["n"], p, NC.LEARN_LEN, seed=NC.LEARN_SEED)
        if cfg == "m6":
            om = C.Model(C.Code(cc["gen1"], 6, 1, 2), p, NC.LEARN_LEN, 200, 1.0, NC.LEARN_SEED)
            assert om.kind == 1 == host.info()["kind"]
            lp, keys = host.rows()
            olp, okeys = om.rows()
            np.testing.assert_array_equal(keys, okeys)
            assert np.array_equal(lp, olp)

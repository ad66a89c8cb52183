"""Chunked detection (csrc/cvd_kernels.hip ck_submit / ck_combine_kernel,
csrc/cvd_k1s.h k1s_wave<XM, true>): a batch too small to fill the device -- the reference's
own call shape, run_experiment with num_iter = 10,000 (Pd_plotter.py:67-75, 199-233) -- has
every sequence's N steps cut into time chunks that start warm-up steps early from D = 0 on
lanes of their own.  A sequence's chunks count only where they join (D at a chunk's start =
the previous chunk's D at its end: the recursion of viterbi_markov.py:139-159 is a function of
D and the word) and its decision (Pd_plotter.py:215, :222) is certain under the rounding
bounds of both summation orders; every other sequence is rerun sequentially.  So the counts
must equal the sequential launch's and the C oracle's EXACTLY -- with chunks that mostly do
not join (no warm-up), with every sequence rerun, ragged N and batches, multi-model launches,
the persistent launch, and at the headline's N = 1e5.

Two kinds of points.  The tests down to test_run_experiment_chunked_equals_unchunked run at
p in [0.01, 0.2] with 2e5-3e5-step models, where the C oracle's counts are [0, T]: every
decision is trivial there, so they check that chunks join and that reruns restore the counts,
not the per-chunk sums.  The tests from test_warm_chunks_informative on are the INFORMATIVE
ones: p = 0.002 (default 1e6-step model) and p = 0.0033 (1e7-step model), where the oracle's
Pd lies strictly inside (0.05, 0.95) -- each asserts so -- and, with gen1 as both hypotheses
("same-code": the H2 half is H1-like with other noise), the H2 count does too.  Their expected
counts are the C oracle's on the same trial ids, so a wrong row lookup, cursor or chunk sum
after a warm start from D = 0 changes a count.  test_near_tie_branch widens the rounding bound
(CVD_CHUNK_KAPPA_LOG2) until about half the sequences are near-ties of ck_combine_kernel."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

SEED = 12345


def _buf(pkg, det, g1, g2, N, p, T, lo=0):
    tag = pkg.grid_tag(N, p)
    r = det.stream_buffer(N, 2 * T)
    det.generate(g1, N, p, SEED, tag, 2 * lo, 2, T, out=r, q0=0, pitch=2 * T)
    det.generate(g2, N, p, SEED, tag, 2 * lo + 1, 2, T, out=r, q0=T, pitch=2 * T)
    return r


@pytest.fixture(scope="module")
def m6(pkg):
    cc = pkg.CONFIG_CODES["m6"]
    det = pkg.Detector(1, 2, 6, cc["gen1"], device=0)
    g1, g2 = pkg.Code(cc["gen1"], 6, 1, 2), pkg.Code(cc["gen2"], 6, 1, 2)
    models = {p: det.model(p, 300_000, 200, 1.0, SEED) for p in (0.01, 0.05, 0.2)}
    return cc, det, g1, g2, models


def _counts(pkg, det, model, r, N, T, **env):
    c = det.detect(model, r, N, 2 * T, T)
    torch.cuda.synchronize()
    return c.cpu().tolist(), pkg._lib.chunk_last()


def _seq_counts(det, model, r, N, T):
    """the unchunked launch's counts (per-sequence sums: sums force the sequential path)"""
    s = torch.empty((2 * T, 2), dtype=torch.float64, device=det.device)
    c = det.detect(model, r, N, 2 * T, T, sums=s)
    s = s.cpu().numpy()
    assert c.cpu().tolist() == [int((s[:T, 0] > s[:T, 1]).sum()), int((s[T:, 0] <= s[T:, 1]).sum())]
    return c.cpu().tolist()


@pytest.mark.parametrize("p,N,T,warm", [(0.05, 20_000, 333, 1152), (0.2, 10_007, 200, 384), (0.01, 20_000, 129, 768),
                                        (0.2, 4_000, 64, 192)])
def test_chunked_counts_equal_sequential(pkg, m6, monkeypatch, p, N, T, warm):
    cc, det, g1, g2, models = m6
    r = _buf(pkg, det, g1, g2, N, p, T)
    ref = _seq_counts(det, models[p], r, N, T)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", str(warm))
    got, st = _counts(pkg, det, models[p], r, N, T)
    assert st["groups"] == 1 and st["C"] >= 2, st
    assert got == ref, (got, ref, st)
    assert models[p].device_error() == 0


def test_chunks_that_do_not_join_are_rerun(pkg, m6, monkeypatch):
    """no warm-up: chunk j starts from D = 0 at its first summed step, so most chunks do not
    join their predecessor; the reruns must restore the exact counts"""
    cc, det, g1, g2, models = m6
    N, T, p = 9_000, 100, 0.2
    r = _buf(pkg, det, g1, g2, N, p, T, lo=5_000)
    ref = _seq_counts(det, models[p], r, N, T)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "0")
    got, st = _counts(pkg, det, models[p], r, N, T)
    assert st["groups"] == 1 and st["reruns"] > T, st
    assert got == ref


def test_every_sequence_rerun(pkg, m6, monkeypatch):
    cc, det, g1, g2, models = m6
    N, T, p = 6_000, 77, 0.05
    r = _buf(pkg, det, g1, g2, N, p, T, lo=9_000)
    ref = _seq_counts(det, models[p], r, N, T)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "384")
    monkeypatch.setenv("CVD_CHUNK_REDO_ALL", "1")
    got, st = _counts(pkg, det, models[p], r, N, T)
    assert st["reruns"] == 2 * T, st
    assert got == ref


def test_chunked_persistent_launch(pkg, m6, monkeypatch):
    """more chunk units than resident slots: the single-model chunked launch is persistent"""
    cc, det, g1, g2, models = m6
    N, T, p = 12_000, 300, 0.05
    r = _buf(pkg, det, g1, g2, N, p, T, lo=20_000)
    ref = _seq_counts(det, models[p], r, N, T)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "192")
    monkeypatch.setenv("CVD_K1S_PERSIST_BLOCKS", "3")   # a tiny persistent grid: the queue drains every unit
    got, st = _counts(pkg, det, models[p], r, N, T)
    assert st["C"] >= 2
    assert got == ref


def test_chunked_multi_model_launch(pkg, m6, monkeypatch):
    """a p row in cvd_detect_multi: the LDS-filter model (p = 0.01) and the others in chunked
    groups; every model's counts equal its sequential launch"""
    cc, det, g1, g2, models = m6
    N = 15_000
    ps, T = [0.01, 0.05, 0.2], [129, 200, 64]
    bufs = [_buf(pkg, det, g1, g2, N, p, t, lo=30_000) for p, t in zip(ps, T)]
    ref = [_seq_counts(det, models[p], r, N, t) for p, r, t in zip(ps, bufs, T)]
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "768")
    cnts = [torch.zeros(2, dtype=torch.int64, device=det.device) for _ in ps]
    det.detect_multi([models[p] for p in ps], bufs, N, [2 * t for t in T], T, cnts)
    st = pkg._lib.chunk_last()
    assert st["groups"] >= 2, st     # the LDS-filter variant apart from the others
    assert [c.cpu().tolist() for c in cnts] == ref


def test_chunked_headline_N_equals_c_oracle(pkg, m6):
    """the default (automatic) chunking at the headline's N = 1e5: counts = the C oracle's"""
    cc, det, g1, g2, models = m6
    N, T, p, lo = 100_000, 256, 0.05, 3_000_000
    res = det.run_trials(models[p], cc["gen1"], cc["gen2"], N, p, SEED, lo, lo + T)
    torch.cuda.synchronize()
    st = pkg._lib.chunk_last()
    assert st["groups"] == 1 and st["C"] >= 2, st
    c1, c2 = C.Code(cc["gen1"], 6, 1, 2), C.Code(cc["gen2"], 6, 1, 2)
    cnt, _ = C.Model(c1, p, 300_000, 200, 1.0, SEED).run_trials(c1, c2, N, p, SEED, lo, lo + T, nthreads=16)
    assert res["counts"].cpu().tolist() == [int(x) for x in cnt]


def test_run_experiment_chunked_equals_unchunked(pkg, monkeypatch):
    """the reference's call shape through the drop-in (cvd_mc_run_grid -> cvd_detect_multi):
    the DataFrame with chunking equals the one without"""
    cc = pkg.CONFIG_CODES["m6"]
    args = (1, 2, 6, cc["gen1"], cc["gen2"], 300, [0.02, 0.1], 200_000, 200, 1.0, SEED)
    monkeypatch.setenv("CVD_CHUNK", "0")
    df0 = pkg.run_experiment(*args, N_list=[30_000], early_decision=False)
    monkeypatch.setenv("CVD_CHUNK", "-1")
    df1 = pkg.run_experiment(*args, N_list=[30_000], early_decision=False)
    assert pkg._lib.chunk_last()["groups"] >= 1
    assert df0.equals(df1), (df0, df1)


# ──────────── informative points: 0.05 < Pd < 0.95 in the C oracle ────────────

class _Point:
    """One p of the m = 6 pair: the model on the GPU and in the C oracle, and the oracle's
    counts and per-trial sums by trial range (computed once, read-only)."""

    def __init__(self, m6, p, learn_len):
        self.cc, self.det, self.g1, self.g2, _ = m6
        self.p, self.learn_len = p, learn_len
        self.model = self.det.model(p, learn_len, 200, 1.0, SEED)
        self.c1, self.c2 = C.Code(self.cc["gen1"], 6, 1, 2), C.Code(self.cc["gen2"], 6, 1, 2)
        self.cm = C.Model(self.c1, p, learn_len, 200, 1.0, SEED)
        self._ref = {}

    def oracle(self, N, lo, hi, same):
        """([s1, s2], sums [T, 4]) of trials lo..hi; same: gen1 as both hypotheses"""
        key = (N, lo, hi, same)
        if key not in self._ref:
            cnt, s = self.cm.run_trials(self.c1, self.c1 if same else self.c2, N, self.p, SEED, lo, hi, sums=True,
                                        nthreads=16)
            s.setflags(write=False)
            self._ref[key] = ([int(x) for x in cnt], s)
        return self._ref[key]

    def chunked(self, pkg, N, lo, hi, same):
        """the counts-only detect call over the same trials (chunked under the caller's CVD_CHUNK*)"""
        T = hi - lo
        r = _buf(pkg, self.det, self.g1, self.g1 if same else self.g2, N, self.p, T, lo=lo)
        got, st = _counts(pkg, self.det, self.model, r, N, T)
        assert self.model.device_error() == 0
        return got, st


@pytest.fixture(scope="module")
def pt002(m6):
    return _Point(m6, 0.002, None)          # the default 1e6-step model


@pytest.fixture(scope="module")
def pt0033(m6):
    return _Point(m6, 0.0033, 10_000_000)


def _informative(ref, T, same):
    assert 0.05 < ref[0] / T < 0.95, ref
    if same:
        assert 0.05 < ref[1] / T < 0.95, ref


def _was_chunked(st, C=None, L=None):
    print("chunk_last", st)   # (DESIGN.md §7.8 records these)
    assert st["groups"] >= 1 and st["C"] >= 2, st
    if C is not None:
        assert (st["C"], st["L"]) == (C, L), st


@pytest.mark.parametrize("same,lo,hi", [(False, 5000, 6024), (True, 5000, 6024), (True, 5000, 6000)])
def test_warm_chunks_informative(pkg, pt002, monkeypatch, same, lo, hi):
    """N = 3,000 in 16 chunks of 192: chunks 2-15 start 384 steps early from D = 0, the last has
    120 steps; T = 1000 puts H1 and H2 lanes into one wave and leaves the last wave ragged.  The
    same-code chunks all join by 192 steps in the oracle, so the chunk sums decide the counts."""
    N, T = 3_000, hi - lo
    ref, _ = pt002.oracle(N, lo, hi, same)
    _informative(ref, T, same)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "384")
    got, st = pt002.chunked(pkg, N, lo, hi, same)
    _was_chunked(st, 16, 192)
    assert got == ref, (got, ref, st)
    if same:
        assert st["reruns"] <= 0.05 * 2 * T, st


@pytest.mark.parametrize("N", [1_153, 1_157])
@pytest.mark.parametrize("same", [False, True])
def test_last_chunk_shorter_than_six_steps(pkg, pt002, monkeypatch, N, same):
    """N = 6 * 192 + 1 and + 5: the seventh chunk is a tail block of one and of five steps"""
    lo, hi = 0, 2_048
    ref, _ = pt002.oracle(N, lo, hi, same)
    _informative(ref, hi - lo, same)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "192")
    got, st = pt002.chunked(pkg, N, lo, hi, same)
    _was_chunked(st, 7, 192)
    assert got == ref, (got, ref, st)


@pytest.mark.parametrize("same,warm", [(True, 0), (False, 192)])
def test_reruns_mixed_with_kept_informative(pkg, pt002, monkeypatch, same, warm):
    """decided + rerun sequences partition the batch (no double count, no drop): the pair at 192
    warm-up steps, where ~12% of the H2 restarts have not joined (every H1 restart has after 33
    steps, so the H1 half is kept; measured: 796 of 2,048 rerun), and same-code with no warm-up,
    where informative decisions come from the rerun (measured: all 2,048 rerun)"""
    N, lo, hi = 3_000, 5_000, 6_024
    T = hi - lo
    ref, _ = pt002.oracle(N, lo, hi, same)
    _informative(ref, T, same)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", str(warm))
    got, st = pt002.chunked(pkg, N, lo, hi, same)
    _was_chunked(st, 16, 192)
    assert 0 < st["reruns"], st
    if not same:
        assert st["reruns"] < 2 * T, st
    assert got == ref, (got, ref, st)


def test_near_tie_branch(pkg, pt002, monkeypatch):
    """ck_combine_kernel's d > e / d < -e with the bound widened by 2^k (CVD_CHUNK_KAPPA_LOG2) so
    that a quarter to three quarters of the joined sequences fall inside it and are rerun; k is
    taken where no oracle gap ratio is within 1e-6 of the threshold (chunk-order sums differ from
    the oracle's by ~1e-13 relative), so the number inside is known exactly."""
    N, lo, hi = 3_000, 5_000, 6_024
    T = hi - lo
    ref, sums = pt002.oracle(N, lo, hi, True)
    _informative(ref, T, True)
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "768")
    monkeypatch.setenv("CVD_CHUNK_KAPPA_LOG2", "0")
    got, st = pt002.chunked(pkg, N, lo, hi, True)
    _was_chunked(st)
    assert got == ref, (got, ref, st)
    r0 = st["reruns"]
    assert r0 <= 0.05 * 2 * T, st
    s = np.concatenate([sums[:, :2], sums[:, 2:]])
    rho = np.abs(s[:, 0] - s[:, 1]) / (np.abs(s[:, 0]) + np.abs(s[:, 1]))
    kappa = 4.0 * float(N + st["L"] + st["C"] + 16) * 2.0 ** -53    # ck_submit
    ks = [k for k in range(28, 39)
          if 0.25 * 2 * T <= (rho <= 2 * kappa * 2.0 ** k).sum() <= 0.75 * 2 * T
          and np.abs(rho / (2 * kappa * 2.0 ** k) - 1).min() > 1e-6]
    assert ks, (kappa, np.sort(rho)[[0, T // 2, T, 3 * T // 2, -1]])
    k = min(ks, key=lambda k: abs(int((rho <= 2 * kappa * 2.0 ** k).sum()) - T))   # nearest to half
    inside = int((rho <= 2 * kappa * 2.0 ** k).sum())
    monkeypatch.setenv("CVD_CHUNK_KAPPA_LOG2", str(k))
    got, st = pt002.chunked(pkg, N, lo, hi, True)
    print("k", k, "inside", inside, "r0", r0)
    _was_chunked(st)
    assert got == ref, (got, ref, k, st)
    assert inside <= st["reruns"] <= inside + r0, (k, inside, r0, st)


def test_chunked_multi_model_informative(pkg, m6, pt002, pt0033, monkeypatch):
    """cvd_detect_multi over two informative models and a trivial one (p = 0.05) in one call"""
    cc, det, g1, g2, models = m6
    N = 3_000
    trials = [(5_000, 6_024), (0, 512), (0, 64)]
    ref = [pt002.oracle(N, *trials[0], False)[0], pt0033.oracle(N, *trials[1], False)[0]]
    for c, (lo, hi) in zip(ref, trials):
        _informative(c, hi - lo, False)
    cnt, _ = C.Model(pt002.c1, 0.05, 300_000, 200, 1.0, SEED).run_trials(pt002.c1, pt002.c2, N, 0.05, SEED, *trials[2],
                                                                       nthreads=16)
    ref.append([int(x) for x in cnt])
    ps, mods = [0.002, 0.0033, 0.05], [pt002.model, pt0033.model, models[0.05]]
    T = [hi - lo for lo, hi in trials]
    bufs = [_buf(pkg, det, g1, g2, N, p, t, lo=lo) for p, t, (lo, _) in zip(ps, T, trials)]
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "384")
    cnts = [torch.zeros(2, dtype=torch.int64, device=det.device) for _ in ps]
    det.detect_multi(mods, bufs, N, [2 * t for t in T], T, cnts)
    torch.cuda.synchronize()
    st = pkg._lib.chunk_last()
    _was_chunked(st)
    assert [c.cpu().tolist() for c in cnts] == ref, st
    assert all(m.device_error() == 0 for m in mods)


def test_automatic_chunking_headline_N_informative(pkg, pt0033, monkeypatch):
    """the default (automatic) plan at N = 1e5, same-code through run_trials"""
    for v in ("CVD_CHUNK", "CVD_CHUNK_WARM", "CVD_CHUNK_UNITS", "CVD_CHUNK_REDO_ALL", "CVD_CHUNK_KAPPA_LOG2"):
        monkeypatch.delenv(v, raising=False)
    N, T, p = 100_000, 96, pt0033.p
    ref, _ = pt0033.oracle(N, 0, T, True)
    _informative(ref, T, True)
    gen1 = pt0033.cc["gen1"]
    res = pt0033.det.run_trials(pt0033.model, gen1, gen1, N, p, SEED, 0, T)
    torch.cuda.synchronize()
    st = pkg._lib.chunk_last()
    _was_chunked(st)
    assert res["counts"].cpu().tolist() == ref, st
    assert pt0033.model.device_error() == 0


def test_run_experiment_informative_chunked_equals_unchunked(pkg, pt002, monkeypatch):
    """the drop-in where Pd is neither 0 nor 1: the same DataFrame with and without chunking,
    and its Pd and Pc the C oracle's.  The automatic plan keeps chunks of >= 3 warm-ups, so at
    the default 1,152 it leaves N = 3,000 whole (groups = 0); 384 warm-up steps -- enough for the
    pair's H2 restarts to join -- give three chunks of 1,152."""
    cc = pkg.CONFIG_CODES["m6"]
    T, N = 1_000, 3_000
    args = (1, 2, 6, cc["gen1"], cc["gen2"], T, [0.002], 1_000_000, 200, 1.0, SEED)
    monkeypatch.setenv("CVD_CHUNK_WARM", "384")
    monkeypatch.setenv("CVD_CHUNK", "0")
    df0 = pkg.run_experiment(*args, N_list=[N], early_decision=False)
    assert pkg._lib.chunk_last()["groups"] == 0
    monkeypatch.setenv("CVD_CHUNK", "-1")
    df1 = pkg.run_experiment(*args, N_list=[N], early_decision=False)
    _was_chunked(pkg._lib.chunk_last())
    assert df0.equals(df1), (df0, df1)
    assert 0.05 < df1["Pd"][0] < 0.95, df1
    ref, _ = pt002.oracle(N, 0, T, False)
    assert (df1["Pd"][0], df1["Pc"][0]) == (ref[0] / T, (ref[0] + ref[1]) / (2 * T)), (df1, ref)

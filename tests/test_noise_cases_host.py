"""The conditions on tests/noise_cases.py that test_gpu_noise_depths.py relies on, checked where
no GPU is needed: every crafted threshold flips or keeps exactly its target bit in the numpy
restatement's and the C oracle's streams, depth_histogram is a brute-force count, the target
sets see both outcomes at every depth, and the committed edge and learning cases are what
they are said to be."""
import numpy as np
import pytest

import noise_cases as NC
from oracle import c_oracle as C
from oracle import philox
from oracle import restatement as R

M6 = [[[1, 0, 1, 1, 0, 1, 1]], [[1, 1, 1, 1, 0, 0, 1]]]                   # (133, 171), delay order
K1N3 = [[[1, 0, 1, 1, 1]], [[1, 1, 0, 1, 1]], [[1, 1, 1, 1, 1]]]           # test_gpu_parity.py's k1n3
CODES = {2: (1, 2, 6, M6), 3: (1, 3, 4, K1N3)}


def test_crafted_thresholds_are_what_they_say():
    rng = np.random.default_rng(3)
    for u in [0, 1, NC.MASK32, NC.MASK32 - 1, 1 << 31] + [int(x) for x in rng.integers(0, 2 ** 32, 200)]:
        for d in range(1, 33):
            for comp in (False, True):
                thr, f = NC.crafted(u, d, comp)
                assert 0 <= thr <= NC.MASK32 and NC.depth_of(u, thr) == d and f == int(u < thr)
                assert NC.p_of(thr) * 2 ** 32 == thr
            if d < 32:   # the two fillings differ in every bit below plane d
                assert NC.crafted(u, d)[0] ^ NC.crafted(u, d, True)[0] == (1 << (32 - d)) - 1
        assert NC.depth_of(u, NC.crafted_equal(u)[0]) == 33
        if u < NC.MASK32:
            thr, f = NC.crafted_above(u)
            assert thr == u + 1 and f == 1 and NC.depth_of(u, thr) == 33 - ((u ^ thr).bit_length())
        assert len(NC.all_cases(u)) == 64 + 1 + (u < NC.MASK32)
    assert [lab for lab, _, _ in NC.deep_cases(5)] == [f"d{d}o" for d in NC.DEEP_DEPTHS] + ["equal"]


@pytest.mark.parametrize("n", [2, 3])
def test_crafted_cases_set_exactly_the_target_bit_in_both_oracles(n):
    """(1) R.received_stream and C.stream, relative to the p = 0 stream"""
    k, _, m, taps = CODES[n]
    code = C.Code(taps, m, k, n)
    N, spw = NC.N_SHORT[n], 32 // n
    for (q, w, b) in NC.TARGETS[n] + [NC.TARGET_HI]:
        sid = NC.seq_of(q, NC.BASE_HI if (q, w, b) == NC.TARGET_HI else NC.BASE)
        t, j = w * spw + b // n, b % n
        assert t < N and b < spw * n
        u = NC.uniform_of(NC.SEED, NC.TAG, sid, w, b)
        clean = R.received_stream(taps, m, k, n, N, 0.0, NC.SEED, NC.TAG, sid)
        np.testing.assert_array_equal(C.stream(code, N, 0.0, NC.SEED, NC.TAG, sid), clean)
        for label, thr, flips in NC.all_cases(u):
            p = NC.p_of(thr)
            r = R.received_stream(taps, m, k, n, N, p, NC.SEED, NC.TAG, sid)
            c = C.stream(code, N, p, NC.SEED, NC.TAG, sid)
            assert ((int(r[t]) ^ int(clean[t])) >> j) & 1 == flips, (q, w, b, label, "restatement")
            assert ((int(c[t]) ^ int(clean[t])) >> j) & 1 == flips, (q, w, b, label, "C oracle")
            np.testing.assert_array_equal(c, r)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_depth_histogram_is_the_brute_force_count(n):
    """(2) on 37 sequences (two of them past 2^32) of 11 words, at thresholds that leave deep bits"""
    seed, tag, nwords, spw = 77, 0x1234567, 11, 32 // n
    sids = list(range(5, 5 + 3 * 35, 3)) + [2 ** 33 + 7, 2 ** 45 + 1]
    u0 = NC.uniform_of(seed, tag, sids[4], 7, 2)
    for thr in (philox.threshold(0.05), 0, NC.MASK32, u0, NC.crafted(u0, 30)[0], NC.crafted(u0, 17, True)[0]):
        hist, deep = NC.depth_histogram(seed, tag, sids, nwords, n, thr, deep_from=12, block=64)
        assert np.array_equal(hist, NC.depth_histogram(seed, tag, sids, nwords, n, thr))
        want, want_deep = np.zeros(34, np.int64), []
        for sid in sids:
            us = philox.noise_word_uniforms(seed, tag, sid, np.arange(nwords), n)
            for w in range(nwords):
                for b in range(spw * n):
                    d = NC.depth_of(int(us[w, b]), thr)
                    want[d] += 1
                    if d >= 12:
                        want_deep.append((sid, w, b, d))
        assert np.array_equal(hist, want) and hist.sum() == len(sids) * nwords * spw * n
        assert sorted(deep) == sorted(want_deep)
        if thr == u0:
            assert (sids[4], 7, 2, 33) in deep
        if thr == 0:   # decided at u's first set bit
            assert hist[33] == sum(1 for e in deep if e[3] == 33)


@pytest.mark.parametrize("n", [2, 3])
def test_target_sets_see_both_outcomes_at_every_depth(n):
    """(3) and the structure the GPU test names: lanes, words, bits"""
    tg = NC.TARGETS[n]
    spw, N = 32 // n, NC.N_SHORT[n]
    nwords = -(-N // spw)
    assert nwords == 9 and NC.COUNT == 130
    assert {q for q, _, _ in tg} >= {0, 63, 64, 127, 128, 129}
    assert {w % 4 for _, w, _ in tg} == {0, 1, 2, 3} and any(w == nwords - 1 for _, w, _ in tg)
    assert {b for _, _, b in tg} >= {0, spw * n - 1}
    for (q, w, b) in tg + [NC.TARGET_HI]:
        live = min(spw, N - w * spw) * n
        assert 0 <= q < NC.COUNT and 0 <= w < nwords and 0 <= b < live
    us = [NC.uniform_of(NC.SEED, NC.TAG, NC.seq_of(q), w, b) for q, w, b in tg]
    for d in range(1, 33):
        assert {NC.crafted(u, d)[1] for u in us} == {0, 1}, d
        assert {NC.crafted(u, d, True)[1] for u in us} == {0, 1}, d
    assert all(0 < u < NC.MASK32 for u in us)
    if n == 2:
        q, w, b = NC.TARGET_LONG
        assert w == -(-NC.N_LONG // 16) - 1 and w % 4 == 0 and b < 2 * (NC.N_LONG - 16 * w)


def test_edges_and_learning_target():
    assert [philox.threshold(p) for p in NC.EDGE_P] == NC.EDGE_THR
    w, b, u = NC.learn_target()
    assert 13 <= w and 16 * w + b // 2 < NC.LEARN_LEN
    assert u == NC.uniform_of(NC.LEARN_SEED, philox.LEARN_TAG, 0, w, b)
    for thr in (NC.crafted(u, 32)[0], NC.crafted_equal(u)[0]):
        assert 0.01 <= NC.p_of(thr) <= 0.2 and NC.depth_of(u, thr) >= 32

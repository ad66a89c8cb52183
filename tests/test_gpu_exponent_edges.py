"""Edge shapes of the error-exponent engine (csrc/cvd_exponent.hip) through the C ABI,
against the high-precision references of oracle/exponent.py on the inputs of
tests/exponent_cases.py (tests/test_exponent_reference_host.py shows those inputs to lie
within the references' limits).

A  the two build kernels element by element against mpmath.  Bounds (eps = 2^-52), derived:
   p = (c + lam) / rs carries three roundings, the exponents are <= 1, each pow is within
   2 ulp, then one multiply and one subtract, so |vals - ref| <= 16 eps (T + T0),
   |a - ref| <= 16 eps a, and the R-term dense sum s within (16 + R) eps s.
B  the certified bracket of cvd_spectral_radius contains the true root: every row sum of
   E nonnegative terms has relative error <= E eps, so lo (1 - (E + 4) eps) <= hi_ref and
   hi (1 + (E + 4) eps) >= lo_ref for perron_bracket's (lo_ref, hi_ref); the HBM path
   against the LDS path; exact scale invariance; bit-identical repeats.
C  no silent wrong answer: whenever the returned bounds are finite and meet tol the value
   is rho to 1e-11, and the Python wrappers return rho to 1e-11 for any nonnegative matrix.
D  cvd_count_transitions at its launch-shape edges against the oracle's automaton walk."""
import ctypes
import sys

import numpy as np
import pytest
import torch

import exponent_cases as XC
from conftest import code_of
from oracle import exponent as OE
from oracle import restatement as R

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
RTOL_RHO, RTOL_I = 1e-11, 1e-10      # the project's (test_gpu_exponent.py)
TOL, MAX_ITER = 1e-13, 200_000
CVD_OK, CVD_E_INVALID = 0, -1
SENTINEL = -777.0


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(x, dtype=torch.float64):
    """A flat device copy; the caller keeps it alive until the call that reads it has run."""
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device="cuda").reshape(-1)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def raw_build(pkg, c1, c2, lam, u):
    """cvd_chernoff_build itself: (rc, a [U, K], vals [U, K, R])."""
    K, R = c1.shape
    U = len(u)
    a = torch.full((U * K,), SENTINEL, dtype=torch.float64, device="cuda")
    vals = torch.full((U * K * R,), SENTINEL, dtype=torch.float64, device="cuda")
    d1, d2, du = _dev(c1), _dev(c2), _dev(u)
    rc = pkg.lib().cvd_chernoff_build(K, R, _ptr(d1), _ptr(d2), float(lam), _ptr(du), U, _ptr(a), _ptr(vals), _stream())
    torch.cuda.synchronize()
    return rc, a.view(U, K).cpu().numpy(), vals.view(U, K, R).cpu().numpy()


def raw_build_dense(pkg, P1, P2, u):
    K, R = P1.shape[0], P1.shape[2]
    U = len(u)
    vals = torch.full((U * K * K,), SENTINEL, dtype=torch.float64, device="cuda")
    d1, d2, du = _dev(P1), _dev(P2), _dev(u)
    rc = pkg.lib().cvd_chernoff_build_dense(K, R, _ptr(d1), _ptr(d2), _ptr(du), U, _ptr(vals), _stream())
    torch.cuda.synchronize()
    return rc, vals.view(U, K, K).cpu().numpy()


def raw_rho(pkg, K, E, a, vals, cols, U, tol=TOL, max_iter=MAX_ITER):
    """cvd_spectral_radius itself: (rc, out [U, 3] = estimate, lower, upper, iters [U])."""
    rho = torch.full((3 * max(U, 1),), SENTINEL, dtype=torch.float64, device="cuda")
    its = torch.full((max(U, 1),), -7, dtype=torch.int32, device="cuda")
    da, dv, dc = _dev(a), _dev(vals), _dev(cols, torch.int32)
    rc = pkg.lib().cvd_spectral_radius(K, E, _ptr(da), _ptr(dv), _ptr(dc), U, float(tol), int(max_iter), _ptr(rho),
                                       _ptr(its), _stream())
    torch.cuda.synchronize()
    return rc, rho.view(-1, 3).cpu().numpy(), its.cpu().numpy()


def certified(out, tol=TOL):
    lo, hi = out[:, 1], out[:, 2]
    with np.errstate(invalid="ignore"):
        return np.isfinite(lo) & np.isfinite(hi) & (hi - lo <= tol * hi)


# ───────────────────── A: the build kernels against mpmath, element-wise ─────────────────────

@pytest.mark.parametrize("shape", list(XC.STRUCTURED), ids=str)
def test_structured_build_vs_mpmath(pkg, shape):
    c1, c2, lam, u = XC.structured_case(*shape)
    rc, a, vals = raw_build(pkg, c1, c2, lam, u)
    assert rc == CVD_OK
    worst_v = worst_a = 0.0
    for q, uq in enumerate(u):
        ra, rv, T, T0 = OE.mp_structured_build(c1, c2, lam, uq)
        worst_a = max(worst_a, float(np.max(np.abs(a[q] - ra) / (EPS * ra))))
        worst_v = max(worst_v, float(np.max(np.abs(vals[q] - rv) / (EPS * (T + T0[:, None])))))
        zero = ~c1.any(axis=1) & ~c2.any(axis=1)
        assert zero.any() and np.all(vals[q][zero] == 0.0)     # all-zero rows: exactly 0.0
        assert np.all(rv[zero] == 0.0)
    print(f"structured build {shape}: worst |a - ref| = {worst_a:.2f} eps a, "
          f"worst |vals - ref| = {worst_v:.2f} eps (T + T0)")
    assert worst_a <= 16 and worst_v <= 16


@pytest.mark.parametrize("shape", list(XC.DENSE), ids=str)
def test_dense_build_vs_mpmath(pkg, shape):
    K, Rr, U = shape
    P1, P2, u = XC.dense_case(*shape)
    rc, vals = raw_build_dense(pkg, P1, P2, u)
    assert rc == CVD_OK
    worst = 0.0
    for q, uq in enumerate(u):
        ref = OE.mp_dense_build(P1, P2, uq)
        worst = max(worst, float(np.max(np.abs(vals[q] - ref) / (EPS * ref))))
    print(f"dense build {shape}: worst |s - ref| = {worst:.2f} eps s (bound {16 + Rr})")
    assert worst <= 16 + Rr


def test_build_argument_errors(pkg):
    c = np.ones((2, 2))
    u = np.array([0.5])
    for lam in (0.0, -1.0, float("nan")):
        rc, a, vals = raw_build(pkg, c, c, lam, u)
        assert rc == CVD_E_INVALID and np.all(a == SENTINEL) and np.all(vals == SENTINEL)
    L = pkg.lib()
    out = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    d, du = _dev(c), _dev(u)
    assert L.cvd_chernoff_build(0, 2, _ptr(d), _ptr(d), 1.0, _ptr(du), 1, _ptr(out), _ptr(out), _stream()) == CVD_E_INVALID
    assert L.cvd_chernoff_build_dense(0, 2, _ptr(d), _ptr(d), _ptr(du), 1, _ptr(out), _stream()) == CVD_E_INVALID
    assert b"chernoff_build_dense" in L.cvd_last_error()
    # U = 0: CVD_OK and nothing is written
    assert L.cvd_chernoff_build(2, 2, _ptr(d), _ptr(d), 1.0, _ptr(None), 0, _ptr(out), _ptr(out), _stream()) == CVD_OK
    P = _dev(np.ones((2, 2, 1)))
    assert L.cvd_chernoff_build_dense(2, 1, _ptr(P), _ptr(P), _ptr(None), 0, _ptr(out), _stream()) == CVD_OK
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)


def test_spectral_radius_argument_errors(pkg, monkeypatch):
    vals = np.ones((2, 2))
    cols = np.zeros((2, 2), np.int32)
    for force in ("0", "1"):
        monkeypatch.setenv("CVD_RHO_GLOBAL", force)
        rc, out, its = raw_rho(pkg, 0, 2, None, vals, cols, 1)
        assert rc == CVD_E_INVALID and np.all(out == SENTINEL) and np.all(its == -7)
        rc, out, its = raw_rho(pkg, 2, 1, None, vals, None, 1)          # dense rows need E = K
        assert rc == CVD_E_INVALID and np.all(out == SENTINEL)
        rc, out, its = raw_rho(pkg, 2, 2, None, vals, cols, 0)          # U = 0 writes nothing
        assert rc == CVD_OK and np.all(out == SENTINEL) and np.all(its == -7)
    monkeypatch.delenv("CVD_RHO_GLOBAL")
    rc, out, its = raw_rho(pkg, 2, 2, None, vals, None, 0)
    assert rc == CVD_OK and np.all(out == SENTINEL) and np.all(its == -7)


# ─────────────────── B: the certified bracket contains the true root ───────────────────

def _check_bracket(out, its, refs, E, what):
    assert np.all(np.isfinite(out)), (what, out)
    assert np.all(out[:, 2] - out[:, 1] <= TOL * out[:, 2]), (what, out)
    assert np.all(its < MAX_ITER) and np.all(its >= 1), (what, its)
    assert np.all(out[:, 1] <= out[:, 0]) and np.all(out[:, 0] <= out[:, 2]), (what, out)
    ld = np.longdouble
    for u, (lo_ref, hi_ref) in enumerate(refs):
        lo, hi = ld(out[u, 1]), ld(out[u, 2])
        assert lo * (1 - ld((E + 4) * EPS)) <= hi_ref, (what, u, out[u], lo_ref, hi_ref)
        assert hi * (1 + ld((E + 4) * EPS)) >= lo_ref, (what, u, out[u], lo_ref, hi_ref)


@pytest.mark.parametrize("fam,K,forced", XC.b_cases(), ids=str)
def test_bracket_contains_root(pkg, monkeypatch, fam, K, forced):
    a, vals, cols = XC.FAMILIES[fam](K)
    U = XC.U_B
    E = K if cols is None else XC.E_ELL
    refs = [OE.perron_bracket(None if a is None else a[u], vals[u], cols, K, E) for u in range(U)]
    monkeypatch.setenv("CVD_RHO_GLOBAL", "1" if forced else "0")
    rc, out, its = raw_rho(pkg, K, E, a, vals, cols, U)
    assert rc == CVD_OK
    _check_bracket(out, its, refs, E, (fam, K, forced))
    if forced and K <= 10232:   # the LDS kernel on the same input: the project's existing bounds
        monkeypatch.setenv("CVD_RHO_GLOBAL", "0")
        rc, lds, ilds = raw_rho(pkg, K, E, a, vals, cols, U)
        assert rc == CVD_OK
        _check_bracket(lds, ilds, refs, E, (fam, K, "lds"))
        np.testing.assert_allclose(out[:, 0], lds[:, 0], rtol=1e-12)
        assert np.all(np.abs(its - ilds) <= 1)


@pytest.mark.parametrize("fam,K,forced", [("structured", 257, False), ("structured", 257, True), ("ell", 1025, False),
                                          ("ell", 1025, True), ("dense", 65, False)], ids=str)
def test_scale_invariance_and_repeat(pkg, monkeypatch, fam, K, forced):
    """One batch of the same matrix scaled by 2^-600, 1, 2^500: (estimate, lower, upper)
    scale exactly and the iteration counts agree (power-of-two scaling commutes with every
    rounding, and each u stops on its own); a second call is bit-identical."""
    a, vals, cols = XC.FAMILIES[fam](K, U=1)
    E = K if cols is None else XC.E_ELL
    s = np.array([2.0 ** -600, 1.0, 2.0 ** 500])
    a3 = None if a is None else a[0][None] * s[:, None]
    v3 = vals[0][None] * s.reshape(3, 1, 1)
    monkeypatch.setenv("CVD_RHO_GLOBAL", "1" if forced else "0")
    rc, out, its = raw_rho(pkg, K, E, a3, v3, cols, 3)
    assert rc == CVD_OK and np.all(certified(out))
    assert its[0] == its[1] == its[2]
    np.testing.assert_array_equal(out[0] / s[0], out[1])
    np.testing.assert_array_equal(out[2] / s[2], out[1])
    rc, again, its2 = raw_rho(pkg, K, E, a3, v3, cols, 3)
    assert rc == CVD_OK and out.tobytes() == again.tobytes() and its.tobytes() == its2.tobytes()


# ───────────────────────────── C: no silent wrong answer ─────────────────────────────

def _close(got, ref):
    return abs(got - ref) <= (RTOL_RHO * ref if ref > 0 else RTOL_RHO)


@pytest.mark.parametrize("forced", [False, True], ids=["lds", "hbm"])
@pytest.mark.parametrize("name", list(XC.NAMED))
def test_named_abi_certified_means_right(pkg, monkeypatch, name, forced):
    M = np.array(XC.NAMED[name][0], np.float64)
    K = len(M)
    ref = OE.eig_rho(M)
    cols = np.tile(np.arange(K, dtype=np.int32), (K, 1)) if forced else None
    monkeypatch.setenv("CVD_RHO_GLOBAL", "1" if forced else "0")
    rc, out, its = raw_rho(pkg, K, K, None, M, cols, 1, max_iter=XC.FAMILY_MAX_ITER)
    assert rc == CVD_OK
    print(f"{name} ({'hbm' if forced else 'lds'}): (est, lo, hi) = {out[0].tolist()}, iters {its[0]}, "
          f"certified {bool(certified(out)[0])}, rho {ref!r}")
    assert 1 <= its[0] <= XC.FAMILY_MAX_ITER
    if certified(out)[0]:
        assert _close(out[0, 0], ref), (name, out[0], ref)
        assert out[0, 1] <= out[0, 0] <= out[0, 2]


def test_family_abi_certified_means_right(pkg, monkeypatch):
    """4,000 sparse nonnegative matrices, one call per K: every certified result is rho, and
    neither share is vacuous (each at least a quarter)."""
    monkeypatch.setenv("CVD_RHO_GLOBAL", "0")
    fam, gold = XC.sparse_family(), XC.family_rho()
    n_cert, wrong = 0, []
    for K in XC.FAMILY_KS:
        U = len(fam[K])
        rc, out, its = raw_rho(pkg, K, K, None, fam[K], None, U, max_iter=XC.FAMILY_MAX_ITER)
        assert rc == CVD_OK and np.all(its >= 1) and np.all(its <= XC.FAMILY_MAX_ITER)
        c = certified(out)
        n_cert += int(c.sum())
        ref = gold[K]
        bad = c & ~(np.abs(out[:, 0] - ref) <= np.where(ref > 0, RTOL_RHO * ref, RTOL_RHO))
        wrong += [(K, int(q), out[q].tolist(), float(ref[q])) for q in np.flatnonzero(bad)]
    print(f"family: {n_cert} of {XC.FAMILY_N} certified, {len(wrong)} of them wrong: {wrong[:4]}")
    assert not wrong
    assert n_cert >= XC.FAMILY_N // 4 and XC.FAMILY_N - n_cert >= XC.FAMILY_N // 4


@pytest.mark.parametrize("name", list(XC.NAMED))
def test_named_spectral_radius(pkg, name):
    M = np.array(XC.NAMED[name][0], np.float64)
    got = pkg.spectral_radius(M, max_iter=XC.FAMILY_MAX_ITER)
    ref = OE.eig_rho(M)
    print(f"{name}: spectral_radius {got!r}, rho {ref!r}")
    assert _close(got, ref), (name, got, ref)


def test_family_spectral_radius(pkg):
    """The first 40 matrices of every K through the Python wrapper."""
    fam, gold = XC.sparse_family(), XC.family_rho()
    wrong = []
    for K in XC.FAMILY_KS:
        for q in range(40):
            got = pkg.spectral_radius(fam[K][q], max_iter=XC.FAMILY_MAX_ITER)
            if not _close(got, gold[K][q]):
                wrong.append((K, q, got, float(gold[K][q])))
    print(f"family through spectral_radius: {len(wrong)} of 200 wrong: {wrong[:6]}")
    assert not wrong


def test_dense_wrappers_on_sparse_unsmoothed_tensors(pkg):
    """Dense Eq. 7 on unsmoothed tensors of two different permutation-like automata: the
    1e-300 clip makes M(u) formally positive but numerically periodic / reducible.  Every
    rho(M(u)) is right and nothing raises."""
    P1, P2 = XC.permutation_tensors()
    K = P1.shape[0]
    u = np.linspace(0.0, 1.0, 11)
    ref = np.array([OE.eig_rho(OE.mp_dense_build(P1, P2, uq)) for uq in u])
    got = pkg.chernoff_rhos(P1, P2, u, max_iter=XC.FAMILY_MAX_ITER)
    out, its = pkg.chernoff_rhos(P1, P2, u, max_iter=XC.FAMILY_MAX_ITER, return_bounds=True)
    print(f"permutation tensors: rho {got.tolist()}, reference {ref.tolist()}, certified {certified(out).tolist()}")
    np.testing.assert_allclose(got, ref, rtol=RTOL_RHO)
    np.testing.assert_array_equal(out[:, 0], got)
    assert not np.all(certified(out))          # the fallback is exercised
    I, ub = pkg.compute_error_exponent(P1, P2, u_grid=11, max_iter=XC.FAMILY_MAX_ITER)
    I_ref, u_ref = OE.compute_error_exponent(P1, P2, 11)
    assert abs(I - (-np.log(ref.min()))) <= RTOL_I * abs(I) and abs(I - I_ref) <= RTOL_I * abs(I_ref)
    if ub != u_ref:
        j, jr = int(np.argmin(np.abs(u - ub))), int(np.argmin(np.abs(u - u_ref)))
        assert abs(ref[j] - ref[jr]) <= RTOL_RHO * ref[jr]
    assert K <= 8   # eig_rho used mpmath


def test_structured_uncertified_raises(pkg):
    """The structured M(u) is positive, so its bracket meets; cut short (max_iter = 1) it is
    uncertified and the wrapper says so instead of returning the norm ratio."""
    c1, c2, lam, _ = XC.structured_case(5, 4, 3)
    nxt = np.random.default_rng(5).integers(0, 5, (5, 4))
    T1, T2 = pkg.TransitionTensor(c1, nxt, lam), pkg.TransitionTensor(c2, nxt, lam)
    with pytest.raises(pkg.CvdError, match=r"u = 0\.5\) is not certified.*bracket \["):
        pkg.chernoff_rhos(T1, T2, [0.5], max_iter=1)
    out, its = pkg.chernoff_rhos(T1, T2, [0.0, 0.5, 1.0], return_bounds=True)
    assert np.all(certified(out)) and np.all(its < MAX_ITER)
    for q, uq in enumerate((0.0, 0.5, 1.0)):
        a, vals, _, _ = OE.mp_structured_build(c1, c2, lam, uq)
        lo, hi = OE.perron_bracket(a, vals, nxt, 5, 4)
        assert abs(out[q, 0] - float(hi)) <= RTOL_RHO * float(hi)


# ───────────────────────── D: cvd_count_transitions launch shapes ─────────────────────────

def _chain(pkg, meta, name, enc, p):
    """(detector, model, encoder taps, automaton next[K, R]) of a decoder / encoder pair."""
    det_mod = sys.modules[pkg.__name__ + ".detector"]
    k, n, m, dec = code_of(meta, name)
    etaps = code_of(meta, enc)[3]
    det = det_mod._detector(k, n, m, dec, None)
    model = det.model(float(p), learn_len=0, learn_burn=0, laplace=1.0, seed=0)
    nxt = pkg.learn_transition_tensor(etaps, dec, m, p, length=64, burn_in=0, seed=1, k=k, n=n)[0].next
    return det, model, etaps, nxt, (k, n, m)


def raw_count(pkg, det, model, etaps, steps, chains, burn, p, seed, cnt):
    """cvd_generate + cvd_count_transitions itself, accumulating into the int64 tensor cnt."""
    r = det.generate(etaps, steps, float(p), seed, pkg.EXPONENT_TAG, 0, 1, chains)
    rc = pkg.lib().cvd_count_transitions(model.handle, _ptr(r), steps, chains, burn, _ptr(cnt), _stream())
    torch.cuda.synchronize()
    return rc


def _oracle_counts(pkg, etaps, knm, nxt, steps, chains, burn, p, seed):
    k, n, m = knm
    want = np.zeros(nxt.shape, np.int64)
    for c in range(chains):
        r = R.received_stream(etaps, m, k, n, steps, p, seed, pkg.EXPONENT_TAG, c)
        want += OE.automaton_counts(r, nxt, burn, 1 << n)
    return want


@pytest.mark.parametrize("name,enc,p,chains,burn,per", [
    ("m2_75", "m2_57", 0.05, 1025, 3, 40),       # two workgroups, the second with one live lane
    ("r23_m4", "r23_m4_b", 0.02, 3, 7, 1000),    # n = 3: 1,007 steps = 100 words of 10 symbols + 7
    ("m2_75", "m2_57", 0.05, 5, 0, 33),          # burn_in = 0
])
def test_count_shapes_vs_oracle(pkg, golden, name, enc, p, chains, burn, per):
    zg, meta = golden
    det, model, etaps, nxt, knm = _chain(pkg, meta, name, enc, p)
    steps = burn + per
    cnt = torch.zeros(nxt.size, dtype=torch.int64, device="cuda")
    assert raw_count(pkg, det, model, etaps, steps, chains, burn, p, 31, cnt) == CVD_OK
    want = _oracle_counts(pkg, etaps, knm, nxt, steps, chains, burn, p, 31)
    got = cnt.view(nxt.shape).cpu().numpy()
    assert got.sum() == chains * per
    np.testing.assert_array_equal(got, want)
    # a second identical call accumulates: the counts double
    assert raw_count(pkg, det, model, etaps, steps, chains, burn, p, 31, cnt) == CVD_OK
    np.testing.assert_array_equal(cnt.view(nxt.shape).cpu().numpy(), 2 * want)


def test_count_burn_in_covers_the_stream(pkg, golden):
    """burn_in >= N: no step counts, d_cnt keeps what it held."""
    zg, meta = golden
    det, model, etaps, nxt, knm = _chain(pkg, meta, "m2_75", "m2_57", 0.05)
    for burn in (43, 44, 10 ** 12):
        cnt = torch.full((nxt.size,), 7, dtype=torch.int64, device="cuda")
        assert raw_count(pkg, det, model, etaps, 43, 1025, burn, 0.05, 31, cnt) == CVD_OK
        assert torch.all(cnt == 7)


# (23,35) vs (35,23), m = 4, rate 1/2: S = 150,743 (test_gpu_exponent.py)
_M4 = ([[[1, 0, 0, 1, 1]], [[1, 1, 1, 0, 1]]], [[[1, 1, 1, 0, 1]], [[1, 0, 0, 1, 1]]])


def test_count_global_kernel_two_blocks(pkg):
    """S >= 4096: 257 chains are two blocks of the global-record kernel, the second with one
    live lane."""
    g1, g2 = _M4
    chains, burn, per = 257, 5, 20
    T, *_ = pkg.learn_transition_tensor(g2, g1, 4, 0.1, length=chains * per, burn_in=burn, seed=5, k=1, n=2,
                                        chains=chains)
    assert T.K == 150_743
    want = _oracle_counts(pkg, g2, (1, 2, 4), T.next, burn + per, chains, burn, 0.1, 5)
    np.testing.assert_array_equal(T.counts, want)

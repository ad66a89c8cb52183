"""The high-precision references of the exponent engine (oracle/exponent.py:
mp_structured_build, mp_dense_build, perron_bracket, eig_rho) against closed forms, the
reference's goldens and each other, and every input of test_gpu_exponent_edges.py
(tests/exponent_cases.py) shown to lie within those references' limits.  CPU only."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import exponent_cases as XC
from conftest import ROOT
from oracle import exponent as OE

GOLD = os.path.join(ROOT, "tests", "golden")
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def egold():
    z = np.load(os.path.join(GOLD, "exponent.npz"))
    with open(os.path.join(GOLD, "exponent.json")) as f:
        return z, json.load(f)


def dyadic_stochastic(K, rng, bits=20):
    """Rows of integers / 2^bits that sum to exactly 1."""
    M = rng.integers(1, (1 << bits) // K, (K, K))
    M[:, -1] += (1 << bits) - M.sum(axis=1)
    assert np.all(M > 0)
    return M / float(1 << bits)


def contains(br, rho, slack=4 * float(np.finfo(np.longdouble).eps)):
    lo, hi = br
    return lo * (1 - slack) <= rho <= hi * (1 + slack) and hi - lo <= 1e-17 * hi


# ─────────────────────────────────── closed forms ───────────────────────────────────

@pytest.mark.parametrize("K", [1, 2, 7, 8, 9, 40])
def test_row_stochastic_has_rho_one(K):
    rng = np.random.default_rng(K)
    S = dyadic_stochastic(K, rng)
    assert np.all(S.sum(axis=1) == 1.0)
    assert contains(OE.perron_bracket(None, S, None, K, K), 1.0)
    assert abs(OE.eig_rho(S) - 1.0) <= 4 * EPS * (1 if K <= 8 else K)
    # D S D^-1 with a power-of-two D is exact in floating point and similar to S
    d = 2.0 ** rng.integers(-20, 21, K)
    A = S * d[:, None] / d[None, :]
    assert contains(OE.perron_bracket(None, A, None, K, K), 1.0)
    if K <= 8:
        assert abs(OE.eig_rho(A) - 1.0) <= 4 * EPS
    # the same matrix in the ELL and rank-one forms of cvd_spectral_radius
    cols = np.tile(np.arange(K, dtype=np.int32), (K, 1))
    assert contains(OE.perron_bracket(None, S, cols, K, K), 1.0)
    a = S.min(axis=1)
    assert contains(OE.perron_bracket(a, S - a[:, None], cols, K, K), 1.0)
    np.testing.assert_array_equal(OE.ell_dense(a, S - a[:, None], cols, K, K), (S - a[:, None]) + a[:, None])


@pytest.mark.parametrize("name", list(XC.NAMED))
def test_named_matrices(name):
    M, rho = XC.NAMED[name]
    M = np.array(M, np.float64)
    got = OE.eig_rho(M)
    if rho is None:   # bipartite: rho^2 is the Perron root of the positive 2 x 2 product of its blocks
        B = M[:2, 2:] @ M[2:, :2]
        rho = float(np.sqrt(OE.perron_bracket(None, B, None, 2, 2)[0]))
        assert abs(rho - 3.7505) < 5e-5
    assert abs(got - rho) <= 4 * EPS * rho, (got, rho)
    assert abs(XC.scc_rho(M) - rho) <= 1e-13 * max(rho, 1.0)
    if name == "triangular":   # reducible, but the dominant class is reached with x > 0
        assert contains(OE.perron_bracket(None, M, None, 2, 2), 3.0)
    if name in ("periodic", "cycle", "bipartite", "jordan", "diag12", "nilpotent"):
        with pytest.raises(RuntimeError):   # outside perron_bracket's domain, and it says so
            OE.perron_bracket(None, M, None, len(M), len(M), max_iter=500)


def test_structured_build_closed_forms():
    """u = 1 gives P1's cells, u = 0 P2's (exact rationals, rounded once); equal tensors
    give P at any u; the clamp: K R laplace + rowsum < 1 divides by 1."""
    c1 = np.array([[3.0, 0.0, 5.0, 2.0 ** 40], [0.0, 0.0, 0.0, 0.0], [7.0, 1.0, 0.0, 0.0]])
    c2 = np.array([[1.0, 2.0, 0.0, 9.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    lam = 2.0 ** -3
    K, R = c1.shape

    def cells(c):
        rs = [max(Fraction(int(c[i].sum())) + K * R * Fraction(lam), 1) for i in range(K)]
        return (np.array([[float((Fraction(int(c[i, r])) + Fraction(lam)) / rs[i]) for r in range(R)]
                          for i in range(K)]),
                np.array([float(Fraction(lam) / rs[i]) for i in range(K)]))

    for u, c in ((1.0, c1), (0.0, c2)):
        a, vals, T, T0 = OE.mp_structured_build(c1, c2, lam, u)
        p, p0 = cells(c)
        np.testing.assert_array_equal(T, p)
        np.testing.assert_array_equal(T0, p0)
        np.testing.assert_array_equal(a, R * p0)
    a, vals, T, T0 = OE.mp_structured_build(c1, c1, lam, 0.25)   # 1 - u is exact
    np.testing.assert_allclose(T, cells(c1)[0], rtol=EPS)
    a, vals, T, T0 = OE.mp_structured_build(c1, c2, lam, 0.5)
    assert np.all(vals[1] == 0.0) and np.all(vals[0] != 0.0)
    np.testing.assert_allclose(T, np.sqrt(cells(c1)[0] * cells(c2)[0]), rtol=4 * EPS)
    # the clamp of the (1, 2, 1) case: rowsum 0 + 0.5 < 1
    c1, c2, lam, u = XC.structured_case(1, 2, 1)
    assert 1 * 2 * lam + c1.sum() < 1
    a, vals, T, T0 = OE.mp_structured_build(c1, c2, lam, u[0])
    assert T0[0] == 0.25 and a[0] == 0.5 and np.all(vals == 0.0)


def test_dense_build_closed_forms():
    P1, P2, _ = XC.dense_case(3, 4, 2)
    np.testing.assert_allclose(OE.mp_dense_build(P1, P2, 1.0), np.clip(P1, 1e-300, 1.0).sum(axis=2), rtol=4 * EPS)
    np.testing.assert_allclose(OE.mp_dense_build(P1, P2, 0.0), np.clip(P2, 1e-300, 1.0).sum(axis=2), rtol=4 * EPS)
    M = OE.mp_dense_build(P1, P1, 0.3)   # p^u p^v = p up to the rounding of v = fl(1 - u)
    np.testing.assert_allclose(M, np.clip(P1, 1e-300, 1.0).sum(axis=2), rtol=700 * EPS)
    one = np.full((1, 1, 1), 1e-320), np.full((1, 1, 1), 2.0)   # both clipped: (1e-300)^u 1^v
    assert OE.mp_dense_build(*one, 0.5)[0, 0] == 1e-150


# ─────────────────────────────── the reference's goldens ───────────────────────────────

def test_rho_goldens(egold):
    z, meta = egold
    for i, want in enumerate(meta["rho"]):
        A = z[f"rho{i}/A"]
        K = len(A)
        assert abs(OE.eig_rho(A) - want) <= 1e-13 * want
        if i == 0:   # this golden is diagonal (reducible): outside perron_bracket's domain
            assert not A[0, 1] and not A[1, 0] and want == A.max()
            continue
        lo, hi = OE.perron_bracket(None, A, None, K, K)
        assert lo * (1 - 1e-13) <= want <= hi * (1 + 1e-13) and hi - lo <= 1e-17 * hi


def _ref_exponent(P1, P2, u_grid):
    """Eq. 7 by mp_dense_build and perron_bracket (the goldens are positive tensors)."""
    K = P1.shape[0]
    best = None
    for u in np.linspace(0.0, 1.0, u_grid):
        rho = float(OE.perron_bracket(None, OE.mp_dense_build(P1, P2, u), None, K, K)[1])
        if best is None or rho < best[0]:
            best = (rho, u)
    return -np.log(best[0]), best[1]


@pytest.mark.parametrize("i", [0, 2])
def test_eq7_goldens(egold, i):
    z, meta = egold
    e = meta["exp"][i]
    P1, P2 = z[f"exp{i}/P1"], z[f"exp{i}/P2"]
    I, u = _ref_exponent(P1, P2, e["u_grid"])
    assert abs(I - e["I_err"]) <= 1e-12 * abs(e["I_err"]) and u == e["u"]
    I2, u2 = OE.compute_error_exponent(P1, P2, e["u_grid"])
    assert abs(I - I2) <= 1e-12 * abs(I2) and u == u2


def test_eq7_golden_points(egold):
    """exp1 (401 u) at a few u: M(u) and rho against the numpy restatement."""
    z, _ = egold
    P1, P2 = z["exp1/P1"], z["exp1/P2"]
    K = P1.shape[0]
    for u in (0.0, 0.1325, 0.535, 1.0):
        M = OE.mp_dense_build(P1, P2, u)
        Mn = np.sum(np.clip(P1, 1e-300, 1) ** u * np.clip(P2, 1e-300, 1) ** (1.0 - u), axis=2)
        np.testing.assert_allclose(Mn, M, rtol=16 * EPS)
        rho = OE.eig_rho(M)
        lo, hi = OE.perron_bracket(None, M, None, K, K)
        assert lo * (1 - 4 * EPS) <= rho <= hi * (1 + 4 * EPS)
        assert abs(rho - np.max(np.abs(np.linalg.eigvals(Mn)))) <= 1e-13 * rho


def test_learned_golden_structured_equals_dense(egold):
    """The structured build of the learned counts, made dense, is the dense build of the
    normalised tensor; its Perron root at the golden u gives the golden I_err."""
    z, meta = egold
    c1, c2, nxt = z["learned/counts1"], z["learned/counts2"], z["learned/next"]
    K, R = c1.shape
    u = meta["learned"]["u"]
    a, vals, T, T0 = OE.mp_structured_build(c1, c2, 1.0, u)
    lo, hi = OE.perron_bracket(a, vals, nxt, K, R)
    assert abs(-np.log(float(hi)) - meta["learned"]["I_err"]) <= 1e-12 * meta["learned"]["I_err"]
    M = OE.mp_dense_build(OE.dense_tensor(c1, nxt, 1.0), OE.dense_tensor(c2, nxt, 1.0), u)
    np.testing.assert_allclose(OE.ell_dense(a, vals, nxt, K, R), M, rtol=64 * EPS)
    assert abs(float(hi) - np.max(np.abs(np.linalg.eigvals(M)))) <= 1e-13 * float(hi)


# ───────────────────── the GPU tests' inputs lie within the references' limits ─────────────────────

@pytest.mark.parametrize("shape", list(XC.STRUCTURED))
def test_structured_inputs_are_exact(shape):
    K, R, U = shape
    c1, c2, lam, u = XC.structured_case(K, R, U)
    assert len(u) == U and c1.shape == c2.shape == (K, R)
    for c in (c1, c2):
        assert np.all(c == np.floor(c)) and np.all(c >= 0) and c.max() <= 2.0 ** 40
        assert c.sum(axis=1).max() < 2.0 ** 53           # row sums are exact in any order
    m, e = np.frexp(lam)
    assert m == 0.5 and lam > 0                          # dyadic
    if K > 3:
        i = np.arange(K)
        assert not c1[i % 7 == 0].any() and not c2[i % 7 == 0].any()
        assert not c1[i % 7 == 1].any() and c2[i % 7 == 1].any()
        assert c1[i % 7 == 2].any() and not c2[i % 7 == 2].any()
        assert c1.max() == 2.0 ** 40 == c2.max()


def test_build_inputs_cover_the_issue():
    us = np.concatenate([u for _, u in XC.STRUCTURED.values()])
    assert {0.0, 1.0, 0.5, 1e-9} <= set(us.tolist())
    assert 2.0 ** -30 in [lam for lam, _ in XC.STRUCTURED.values()]
    for shape in ((3, 4, 2), (17, 8, 3)):
        P1, P2, u = XC.dense_case(*shape)
        for P in (P1, P2):
            assert all(np.any(P == s) for s in XC.DENSE_SPECIALS)


@pytest.mark.parametrize("fam,K,forced", XC.b_cases(), ids=lambda v: str(v))
def test_bracket_inputs_converge(fam, K, forced):
    """perron_bracket meets 1e-17 within its iteration cap on every family member (it raises
    otherwise), and the matrix is what the family says: nonnegative, a > 0 or the cycle and
    the loop present."""
    a, vals, cols = XC.FAMILIES[fam](K)
    E = K if cols is None else XC.E_ELL
    assert np.all(vals >= 0)
    if fam == "structured":
        assert np.all(a > 0)
    if fam == "ell":
        assert np.all(vals > 0) and np.all(cols[:, 0] == np.arange(K)) and np.all(cols[:, 1] == (np.arange(K) + 1) % K)
    if fam == "dense":
        assert np.all(vals > 0)
    for u in range(XC.U_B):
        lo, hi = OE.perron_bracket(None if a is None else a[u], vals[u], cols, K, E)
        assert 0 < lo <= hi and hi - lo <= 1e-17 * hi
        if K <= 8:
            rho = OE.eig_rho(OE.ell_dense(None if a is None else a[u], vals[u], cols, K, E))
            assert lo * (1 - 4 * EPS) <= rho <= hi * (1 + 4 * EPS)


def test_family_golden():
    """tests/golden/exponent_family_rho.npy is eig_rho of sparse_family(): every 16th matrix
    recomputed with mpmath, every matrix by strongly connected components."""
    fam, gold = XC.sparse_family(), XC.family_rho()
    assert sum(len(v) for v in fam.values()) == XC.FAMILY_N
    for K in XC.FAMILY_KS:
        assert fam[K].shape == (800, K, K) and gold[K].shape == (800,)
        assert np.all(fam[K] == np.floor(fam[K])) and fam[K].min() == 0 and fam[K].max() == 3
        for q in range(0, 800, 16):
            assert OE.eig_rho(fam[K][q]) == gold[K][q]
        scc = np.array([XC.scc_rho(M) for M in fam[K]])
        np.testing.assert_allclose(scc, gold[K], rtol=1e-13, atol=0)
        assert np.all((gold[K] == 0) | (gold[K] >= 1))   # integer entries: a cycle has weight >= 1


def test_permutation_tensors_are_sparse_and_stochastic():
    P1, P2 = XC.permutation_tensors()
    for P in (P1, P2):
        np.testing.assert_allclose(P.sum(axis=(1, 2)), 1.0, rtol=2 * EPS)
        assert (P > 0).sum() == P.shape[0] * P.shape[2] and P.min() == 0.0

"""Inputs of the exponent engine's edge tests, shared by test_exponent_reference_host.py
(CPU: every input lies within the references' own limits) and test_gpu_exponent_edges.py
(GPU: the kernels against those references).  Everything is seeded and exact: counts are
integers below 2^53, the Laplace constants are dyadic.

`python tests/exponent_cases.py` rewrites tests/golden/exponent_family_rho.npy, the
mpmath.eig spectral radii of the 4,000-matrix family (about 30 s of mpmath; the host test
re-derives a sample with mpmath and all of them by strongly connected components)."""
import os

import numpy as np

GOLDEN_FAMILY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exponent_family_rho.npy")

# ─────────────────────────────── A: the build kernels ───────────────────────────────

# (K, R, U) -> (laplace, u): u covers 0, 1, 0.5 and 1e-9; (1, 2, 1) has K R laplace = 0.5 and
# zero counts, so its row sum is clamped to 1; (257, 8, 2) has laplace = 2^-30
STRUCTURED = {
    (1, 2, 1): (0.25, [1e-9]),
    (5, 4, 3): (1.0, [0.0, 1.0, 0.5]),
    (257, 8, 2): (2.0 ** -30, [1e-9, 0.75]),
    (300, 1, 1): (0.5, [0.3]),
}
DENSE = {
    (1, 1, 1): [0.5],
    (3, 4, 2): [0.0, 1e-9],
    (17, 8, 3): [1.0, 0.5, 0.3],
}
DENSE_SPECIALS = [0.0, 1e-320, 1e-300, 1.0, 2.0, -0.5]   # both clips, a denormal, a negative


def structured_case(K, R, U):
    """(cnt1, cnt2 [K, R] float64 integers, laplace, u [U]).  Row i with i % 7 == 0 is all-zero
    in both tensors, i % 7 == 1 in cnt1 only, i % 7 == 2 in cnt2 only; the other rows mix
    zeros with counts up to 2^40 (exactly 2^40 in row 3 where there is one)."""
    lam, u = STRUCTURED[(K, R, U)]
    rng = np.random.default_rng(1000 * K + 10 * R + U)
    if (K, R, U) == (1, 2, 1):
        z = np.zeros((K, R))
        return z, z.copy(), lam, np.array(u)

    def counts():
        c = np.floor(2.0 ** rng.uniform(0, 40, (K, R)))
        c[rng.random((K, R)) < 0.2] = 0.0
        return c

    c1, c2 = counts(), counts()
    i = np.arange(K)
    c1[(i % 7 == 0) | (i % 7 == 1)] = 0.0
    c2[(i % 7 == 0) | (i % 7 == 2)] = 0.0
    if K > 3:
        c1[3, 0] = 2.0 ** 40
        c2[3, R - 1] = 2.0 ** 40
    return c1, c2, lam, np.array(u)


def dense_case(K, R, U):
    """(P1, P2 [K, K, R], u [U]): uniform (0, 1) entries with DENSE_SPECIALS planted in both
    tensors at seeded places (every special value occurs when K K R >= 6; at (1, 1, 1) the
    pair is (1e-320, 2.0): one entry below and one above the clips)."""
    u = np.array(DENSE[(K, R, U)])
    rng = np.random.default_rng(2000 * K + 10 * R + U)
    P1, P2 = rng.random((K, K, R)), rng.random((K, K, R))
    n = K * K * R
    if n == 1:
        P1[0, 0, 0], P2[0, 0, 0] = 1e-320, 2.0
        return P1, P2, u
    for P in (P1, P2):
        flat = P.reshape(-1)
        where = rng.permutation(n)
        reps = min(3, n // len(DENSE_SPECIALS)) or 1
        for q, s in enumerate(DENSE_SPECIALS * reps):
            flat[where[q % n]] = s
    return P1, P2, u


# ───────────────────── B: positive / irreducible-aperiodic families ─────────────────────

E_ELL = 4
K_LDS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 10232]
K_SWITCH = 10233                      # the first K whose vectors do not fit LDS
K_FORCED = [1, 255, 256, 257, 1025, 65537]
K_DENSE = [1, 2, 65, 1025]
U_B = 3


def structured_family(K, U=U_B):
    """a [U, K] > 0 (the rank-one part: the matrix is positive), vals [U, K, 4] >= 0 with a
    quarter of exact zeros, cols [K, 4] random."""
    rng = np.random.default_rng(31 * K + 1)
    a = rng.uniform(0.5, 1.5, (U, K)) / K
    vals = rng.uniform(0.0, 1.0, (U, K, E_ELL)) * (rng.random((U, K, E_ELL)) < 0.75)
    cols = rng.integers(0, K, (K, E_ELL)).astype(np.int32)
    return a, vals, cols


def ell_family(K, U=U_B):
    """No rank-one part: vals [U, K, 4] in [0.5, 1.5), cols[i] = (i, i + 1 mod K, random,
    random): the cycle makes the matrix irreducible, the loop aperiodic."""
    rng = np.random.default_rng(31 * K + 2)
    vals = rng.uniform(0.5, 1.5, (U, K, E_ELL))
    cols = rng.integers(0, K, (K, E_ELL)).astype(np.int32)
    cols[:, 0] = np.arange(K)
    cols[:, 1] = (np.arange(K) + 1) % K
    return None, vals, cols


def dense_family(K, U=U_B):
    """Dense rows (cols None, E = K): uniform [0, 1) with 30% exact zeros plus 0.05 everywhere
    (positive)."""
    rng = np.random.default_rng(31 * K + 3)
    vals = rng.random((U, K, K)) * (rng.random((U, K, K)) < 0.7) + 0.05
    return None, vals, None


FAMILIES = {"structured": structured_family, "ell": ell_family, "dense": dense_family}


def b_cases():
    """(family, K, forced HBM path) of every bracket test."""
    out = []
    for fam in ("structured", "ell"):
        out += [(fam, K, False) for K in K_LDS + [K_SWITCH]]
        out += [(fam, K, True) for K in K_FORCED]
    out += [("dense", K, False) for K in K_DENSE]
    return out


# ───────────────────────── C: matrices the iteration cannot certify ─────────────────────────

SQ = np.sqrt
NAMED = {   # name -> (matrix, rho)
    "periodic": ([[0, 2], [1, 0]], SQ(2.0)),
    "cycle": ([[0, 1, 0], [0, 0, 2], [4, 0, 0]], 2.0),
    "bipartite": ([[0, 0, 1, 2], [0, 0, 3, 1], [1, 1, 0, 0], [2, 5, 0, 0]], None),   # 3.7505..., by eig_rho
    "early_stop": ([[0, 0, 3, 0], [0, 0, 0, 1], [0, 0, 0, 3], [0, 1, 0, 0]], 1.0),
    "jordan": ([[1, 1], [0, 1]], 1.0),
    "diag12": ([[1, 0], [0, 2]], 2.0),
    "triangular": ([[3, 0], [1, 1]], 3.0),
    "nilpotent": ([[0, 1], [0, 0]], 0.0),
    "zero": ([[0, 0], [0, 0]], 0.0),
    "half": ([[0.5, 0, 0], [1, 0, 1], [0, 0, 0]], 0.5),
    "sqrt6": ([[0, 0, 0, 0, 2, 0], [0, 0, 0, 0, 0, 3], [1, 2, 0, 2, 0, 0], [0, 0, 3, 0, 1, 0],
               [1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], SQ(6.0)),
}

FAMILY_N, FAMILY_KS, FAMILY_MAX_ITER = 4000, (2, 3, 4, 5, 6), 3000


def sparse_family():
    """{K: [800, K, K] float64}: 4,000 random sparse nonnegative matrices, K = 2..6 in turn,
    integer entries 0..3, density uniform in [0.25, 0.6], default_rng(1)."""
    rng = np.random.default_rng(1)
    out = {K: [] for K in FAMILY_KS}
    for q in range(FAMILY_N):
        K = FAMILY_KS[q % len(FAMILY_KS)]
        dens = rng.uniform(0.25, 0.6)
        out[K].append((rng.integers(0, 4, (K, K)) * (rng.random((K, K)) < dens)).astype(np.float64))
    return {K: np.stack(v) for K, v in out.items()}


def family_rho():
    """{K: [800]} the golden mpmath.eig spectral radii of sparse_family()."""
    flat = np.load(GOLDEN_FAMILY)
    per = FAMILY_N // len(FAMILY_KS)
    return {K: flat[q * per:(q + 1) * per] for q, K in enumerate(FAMILY_KS)}


def scc_rho(M):
    """rho of a nonnegative matrix as the largest Perron root of its strongly connected
    components (each a simple eigenvalue of an irreducible block, so np.linalg.eigvals is
    well conditioned there even when M itself is defective)."""
    M = np.asarray(M, np.float64)
    K = M.shape[0]
    reach = (M > 0) | np.eye(K, dtype=bool)
    for _ in range(K):
        reach = reach | ((reach.astype(np.int64) @ reach.astype(np.int64)) > 0)
    both = reach & reach.T
    rho, seen = 0.0, np.zeros(K, bool)
    for i in range(K):
        if not seen[i]:
            idx = np.flatnonzero(both[i])
            seen[idx] = True
            rho = max(rho, float(np.max(np.abs(np.linalg.eigvals(M[np.ix_(idx, idx)])))))
    return rho


def permutation_tensors(K=6, R=2, seed=7):
    """Two sparse unsmoothed transition tensors [K, K, R] of permutation-like automata: for
    each word r the next state is a permutation of the states, P[i, next_r(i), r] = w[i, r]
    with sum_r w[i, r] = 1 and every other cell exactly 0.  The automata share the word-0
    permutation (a K-cycle) and differ in the word-1 permutation."""
    rng = np.random.default_rng(seed)
    cyc = (np.arange(K) + 1) % K
    out = []
    for other in (rng.permutation(K), rng.permutation(K)):
        w = rng.uniform(0.2, 0.8, K)
        P = np.zeros((K, K, R))
        P[np.arange(K), cyc, 0] = w
        P[np.arange(K), other, 1] = 1.0 - w
        out.append(P)
    assert not np.array_equal(out[0] > 0, out[1] > 0)
    return out[0], out[1]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import exponent as OE
    fam = sparse_family()
    np.save(GOLDEN_FAMILY, np.concatenate([[OE.eig_rho(M) for M in fam[K]] for K in FAMILY_KS]))

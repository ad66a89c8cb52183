"""Error-exponent engine, restated for checking (TEST INFRASTRUCTURE ONLY).

Only tests/ may use this module.  Restates alpha_exponent.py's arithmetic
(counts -> normalised tensor :152-154, Eq. 7 via np.linalg.eigvals :69-76,
:159-188, the tail fit :191-215), pinned to the reference's own outputs by
tests/golden/exponent.{npz,json} (tests/golden/make_golden_exponent.py).
"""
import numpy as np


def automaton_counts(r_stream, nxt, burn_in, R):
    """Joint counts [K, R] of (state, received word) along one stream walked on
    the automaton nxt[i, r] from state 0, steps t >= burn_in."""
    K = nxt.shape[0]
    cnt = np.zeros((K, R), np.int64)
    s = 0
    for t, rv in enumerate(r_stream):
        if t >= burn_in:
            cnt[s, rv] += 1
        s = nxt[s, rv]
    return cnt


def dense_tensor(counts, nxt, laplace):
    """alpha_exponent.py:152-154 on C[i, next(i, r), r] = counts[i, r]."""
    K, R = counts.shape
    C = np.zeros((K, K, R), np.float64)
    for i in range(K):
        for r in range(R):
            C[i, nxt[i, r], r] += counts[i, r]
    C += laplace
    C /= np.maximum(C.sum(axis=(1, 2), keepdims=True), 1.0)
    return C


def compute_error_exponent(P1, P2, u_grid=401):
    """alpha_exponent.py:159-188 (numpy eigvals)."""
    P1 = np.clip(P1, 1e-300, 1.0)
    P2 = np.clip(P2, 1e-300, 1.0)
    best_rho = best_u = None
    for u in np.linspace(0.0, 1.0, u_grid):
        M = np.sum((P1 ** u) * (P2 ** (1.0 - u)), axis=2)
        rho = max(float(np.max(np.abs(np.linalg.eigvals(M)))), 1e-300)
        if best_rho is None or rho < best_rho:
            best_rho, best_u = rho, u
    return float(-np.log(best_rho)), float(best_u)


# ───────────── high-precision references of the M(u) builds and of rho ─────────────
# The inputs of the build kernels are doubles and so is the exponent pair: both the
# reference (alpha_exponent.py:175-176) and the kernels raise P1 to u and P2 to the
# double v = fl(1 - u).  The references below take the doubles (u, v) as the data and
# evaluate everything after that exactly (mpmath, MP_DIGITS digits, rounded once): with
# the real number 1 - u in place of v, T would move by |ln p2| * |v - (1 - u)| relative,
# up to 690 * eps / 4 at the clip -- a property of the formula's conditioning, not an
# error of an implementation.

MP_DIGITS = 50
CLIP_LO = 1e-300


def _at_mp_digits(fn):
    """Run fn(mpmath, ...) at MP_DIGITS digits, leaving mpmath's global precision alone."""
    import functools

    @functools.wraps(fn)
    def run(*args, **kw):
        import mpmath
        with mpmath.workdps(MP_DIGITS):
            return fn(mpmath, *args, **kw)
    return run


@_at_mp_digits
def mp_structured_build(mp, cnt1, cnt2, lam, u):
    """cvd_exponent.hip's structured M(u) = a 1^T + V for one u, from joint counts
    cnt1, cnt2 [K, R] and the Laplace constant: rs = max(sum_r cnt + K R lam, 1),
    p = clip((c + lam) / rs, 1e-300, 1), T = p1^u p2^v, T0 the same at c = 0,
    a = R T0, vals = T - T0.  Returns float64 (a[K], vals[K, R], T[K, R], T0[K]),
    each rounded once from MP_DIGITS digits (T and T0 are the scales of the error
    bounds: vals is a difference)."""
    cnt1, cnt2 = np.asarray(cnt1, np.float64), np.asarray(cnt2, np.float64)
    K, R = cnt1.shape
    lam_, u_, v_ = mp.mpf(float(lam)), mp.mpf(float(u)), mp.mpf(1.0 - float(u))
    lo, one = mp.mpf(CLIP_LO), mp.mpf(1)
    a, vals, T, T0 = np.zeros(K), np.zeros((K, R)), np.zeros((K, R)), np.zeros(K)

    def clip(p):
        return min(max(p, lo), one)

    for i in range(K):
        c1 = [mp.mpf(float(c)) for c in cnt1[i]]
        c2 = [mp.mpf(float(c)) for c in cnt2[i]]
        rs1 = max(mp.fsum(c1) + K * R * lam_, one)
        rs2 = max(mp.fsum(c2) + K * R * lam_, one)
        t0 = clip(lam_ / rs1) ** u_ * clip(lam_ / rs2) ** v_
        T0[i], a[i] = float(t0), float(R * t0)
        for r in range(R):
            if cnt1[i, r] == 0 and cnt2[i, r] == 0:
                t = t0
            else:
                t = clip((c1[r] + lam_) / rs1) ** u_ * clip((c2[r] + lam_) / rs2) ** v_
            T[i, r], vals[i, r] = float(t), float(t - t0)
    return a, vals, T, T0


@_at_mp_digits
def mp_dense_build(mp, P1, P2, u):
    """M(u)[i, j] = sum_r clip(P1)^u clip(P2)^v of arbitrary tensors [K, K, R]
    (alpha_exponent.py:171-180), float64 [K, K] rounded once."""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    K, _, R = P1.shape
    u_, v_ = mp.mpf(float(u)), mp.mpf(1.0 - float(u))
    lo, one = mp.mpf(CLIP_LO), mp.mpf(1)
    M = np.zeros((K, K))
    for i in range(K):
        for j in range(K):
            M[i, j] = float(mp.fsum(min(max(mp.mpf(float(P1[i, j, r])), lo), one) ** u_ *
                                    min(max(mp.mpf(float(P2[i, j, r])), lo), one) ** v_ for r in range(R)))
    return M


def ell_dense(a, vals, cols, K, E):
    """The K x K matrix a 1^T + ELL(vals, cols) of cvd_spectral_radius (a None: no
    rank-one part; cols None: dense rows, E = K), as float64."""
    vals = np.asarray(vals, np.float64).reshape(K, E)
    if cols is None:
        M = vals.copy()
    else:
        M = np.zeros((K, K))
        np.add.at(M, (np.repeat(np.arange(K), E), np.asarray(cols).reshape(-1)), vals.reshape(-1))
    if a is not None:
        M += np.asarray(a, np.float64).reshape(K, 1)
    return M


def perron_bracket(a, vals, cols, K, E, rel=1e-17, max_iter=20_000):
    """(lo_ref, hi_ref) with lo_ref <= rho <= hi_ref for the nonnegative matrix
    a 1^T + ELL(vals, cols): the kernels' power iteration with Collatz-Wielandt bounds
    in np.longdouble (64-bit mantissa, pairwise row sums), run until hi - lo <= rel * hi.
    For positive or irreducible-aperiodic matrices; raises if the bracket has not met
    after max_iter iterations or an x_i reaches 0."""
    ld = np.longdouble
    if np.finfo(ld).eps > 2e-19:
        raise RuntimeError("perron_bracket needs an extended-precision np.longdouble")
    V = np.asarray(vals, np.float64).reshape(K, E).astype(ld)
    av = None if a is None else np.asarray(a, np.float64).reshape(K).astype(ld)
    cr = None if cols is None else np.asarray(cols, np.int64).reshape(K, E)
    x = np.ones(K, ld)
    for _ in range(max_iter):
        y = (V * (x[None, :] if cr is None else x[cr])).sum(axis=1)
        if av is not None:
            y = y + av * x.sum()
        if not np.all(x > 0):
            raise RuntimeError("perron_bracket: an x_i reached 0 (not an irreducible matrix?)")
        ratio = y / x
        lo, hi = ratio.min(), ratio.max()
        if hi - lo <= ld(rel) * hi:
            return lo, hi
        x = y / y.max()
    raise RuntimeError(f"perron_bracket: [{lo!r}, {hi!r}] has not met after {max_iter} iterations")


EIG_DIGITS = 120   # a Jordan block of size k moves an eigenvalue by about 10^(-digits / k); k <= 8


def eig_rho(M):
    """max |eigenvalue| of a square matrix: mpmath.eig at EIG_DIGITS digits for K <= 8,
    np.linalg.eigvals above (the reference's spectral_radius).  A nonnegative matrix
    whose pattern is nilpotent has rho = 0 exactly (no rounding of a K-fold zero)."""
    M = np.asarray(M, np.float64)
    K = M.shape[0]
    if K > 8:
        return float(np.max(np.abs(np.linalg.eigvals(M))))
    if K == 1:
        return float(abs(M[0, 0]))
    if np.all(M >= 0) and not np.linalg.matrix_power((M > 0).astype(np.int64), K).any():
        return 0.0
    import mpmath
    with mpmath.workdps(EIG_DIGITS):
        ev = mpmath.eig(mpmath.matrix(M.tolist()), left=False, right=False)
        return float(max(abs(e) for e in ev))

"""Cases of the P̂1 learning chain (csrc/cvd_learn.hip) and their references, built on the
oracles alone.  TEST INFRASTRUCTURE ONLY.

* CODES: one code per kernel instance of the GPU chain -- the six chain_sparse_kernel<m,k,n>
  (m2..m6 at rate 1/2, r23 = <4,2,3>; key widths NW = 1, 1, 2, 4, 8, 2 words) and the three
  chain_dense_kernel<n> (n1, then m2 / m3, then r13 / r23).
* Case + oracle_model / product_model / assert_equals_oracle: a model of the product (host or
  GPU chain) against oracle/cvd_oracle.c, which shares no code with the product.
* expected_mismatches: the number of speculative blocks whose start state is wrong, from the
  Python restatement (oracle/restatement.py) alone -- what LearnStats.mismatched_blocks must
  report after the first verify pass.

test_learn_cases_host.py checks the helpers and that the host chain equals the C oracle at every
case; test_gpu_learn_edges.py runs the same cases through the GPU chain."""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import c_oracle as C
from oracle import philox
from oracle import restatement as R

# taps[j][i][d] multiplies x[d] of input i in output j; d = 0 is the input bit
CODES = {
    "m2": (2, 1, 2, [[[1, 1, 1]], [[1, 0, 1]]]),                               # CONFIG_CODES["m2"]
    "m3": (3, 1, 2, [[[1, 1, 0, 1]], [[1, 1, 1, 1]]]),                         # (15,17)
    "m4": (4, 1, 2, [[[1, 0, 0, 1, 1]], [[1, 1, 1, 0, 1]]]),                   # (23,35)
    "m5": (5, 1, 2, [[[1, 0, 1, 0, 1, 1]], [[1, 1, 1, 1, 0, 1]]]),             # (53,75)
    "m6": (6, 1, 2, [[[1, 0, 1, 1, 0, 1, 1]], [[1, 1, 1, 1, 0, 0, 1]]]),       # CONFIG_CODES["m6"]
    "r23": (4, 2, 3, [[[1, 0, 0, 0, 1], [0, 1, 1, 1, 1]], [[1, 1, 1, 0, 1], [0, 1, 0, 1, 0]],
                      [[0, 1, 1, 0, 0], [1, 1, 0, 1, 0]]]),                    # CONFIG_CODES["r23_m4"]
    "r13": (2, 1, 3, [[[1, 1, 1]], [[1, 0, 1]], [[1, 1, 0]]]),                 # rate 1/3: 10 steps per word
    "n1": (2, 1, 1, [[[1, 1, 1]]]),                                            # k = n = 1: 32 steps per word
}
SPARSE_CODES = ["m2", "m3", "m4", "m5", "m6", "r23"]    # with SPARSE_CAP: chain_sparse_kernel, every instance
DENSE_CODES = ["n1", "m2", "m3", "r13", "r23"]          # with DENSE_CAP: chain_dense_kernel<1>, <2>, <2>, <3>, <3>
SPARSE_CAP, DENSE_CAP = 8, 500_000
SEED = 12345
DENSE_P1_MAX_S = 471                                     # dense_P1 is S x S doubles: compared up to m3's S

# a model: code name, p, learn_len (None: the default length), learn_burn, enum_cap
Case = namedtuple("Case", "code p L burn cap")

# (L, CVD_LEARN_BLOCK, CVD_LEARN_WARM) of the geometry cases, all at p = GEOMETRY_P
GEOMETRY = [(3000, 64, 0), (3000, 1, 0), (2049, 256, 0), (2048, 256, 0), (3000, 300, 16)]
GEOMETRY_CODES = [("m3", SPARSE_CAP), ("m4", SPARSE_CAP), ("m5", SPARSE_CAP), ("r13", DENSE_CAP)]
GEOMETRY_P = 0.05

# every sparse instance: one block, one block and a one-step second block (the default block
# length is 256 here), two-entry sort and scans (L = 1); p = 0.2: nearly every step a first visit
SPARSE_LENGTHS = (1, 2, 255, 256, 257, 3000)
SPARSE_CASES = ([Case(c, 0.05, L, 0, SPARSE_CAP) for c in SPARSE_CODES for L in SPARSE_LENGTHS]
                + [Case(c, 0.2, 3000, 200, SPARSE_CAP) for c in SPARSE_CODES])
# every dense instance: the default length max(5000, 200 S) with the reference's burn-in, and
# lengths around one stream word at n = 3 (10 steps), below one word at n = 1 and 2
DENSE_LENGTHS = (1, 9, 10, 11, 257)
DENSE_CASES = ([Case(c, 0.05, None, 200, DENSE_CAP) for c in DENSE_CODES]
               + [Case(c, 0.05, L, 0, DENSE_CAP) for c in DENSE_CODES for L in DENSE_LENGTHS])
BURN_L = 300
BURN_CASES = [Case(c, 0.05, BURN_L, b, cap) for c, cap in (("m3", SPARSE_CAP), ("r13", DENSE_CAP))
              for b in (0, BURN_L - 1, BURN_L, BURN_L + 5)]
GEOMETRY_CASES = [(Case(c, GEOMETRY_P, L, 0, cap), blen, warm) for c, cap in GEOMETRY_CODES
                  for L, blen, warm in GEOMETRY]
COLLISION_CASE = Case("m4", 0.05, 3000, 0, SPARSE_CAP)      # 1299 distinct keys
DEFAULT_BLEN, DEFAULT_WARM = 256, 512                        # chain_geometry at L <= 2^23

ALL_CASES = list(dict.fromkeys(SPARSE_CASES + DENSE_CASES + BURN_CASES + [g[0] for g in GEOMETRY_CASES]
                               + [COLLISION_CASE]))


def case_id(c):
    return f"{c.code}-{'sparse' if c.cap == SPARSE_CAP else 'dense'}-p{c.p}-L{c.L}-burn{c.burn}"


@functools.lru_cache(maxsize=None)
def oracle_model(case):
    """The C oracle's model of `case` (computed once per case, never modified)."""
    m, k, n, taps = CODES[case.code]
    return C.Model(C.Code(taps, m, k, n), case.p, case.L, case.burn, 1.0, SEED, case.cap)


def product_model(pkg, case, learn_device=None):
    m, k, n, taps = CODES[case.code]
    return pkg.Model(pkg.Code(taps, m, k, n), case.p, case.L, case.burn, 1.0, SEED, case.cap,
                     learn_device=learn_device)


@functools.lru_cache(maxsize=None)
def _host_dense_P1(pkg, case):
    return product_model(pkg, case).dense_P1()


def assert_equals_oracle(pkg, model, case):
    """`model` (a pkg.Model of `case`) is the C oracle's model: kind, S, n_rows, learn_len_eff, the
    keys in row order, log P̂1 bit for bit; dense_P1 as the host chain's for small dense models.
    Returns (info, log P̂1, keys)."""
    om = oracle_model(case)
    inf = model.info()
    S = om.S
    assert (inf["kind"], inf["S"], inf["n_rows"]) == (om.kind, S, S), (case, inf)
    assert inf["learn_len_eff"] == C.lib().oc_model_learn_len(om.h), (case, inf)
    lp, keys = model.rows()
    olp, okeys = om.rows()
    np.testing.assert_array_equal(keys, okeys, err_msg=f"{case}: keys / row order")
    assert np.array_equal(lp, olp), (case, "log P1 differs", int((lp != olp).sum()))
    if inf["kind"] == 0 and S <= DENSE_P1_MAX_S:
        assert np.array_equal(model.dense_P1(), _host_dense_P1(pkg, case)), (case, "dense_P1")
    return inf, lp, keys


def assert_laplace_rows(inf, lp):
    """No step counted (burn >= L): every row is the all-zero-count row, laplace / (S laplace)
    (S additions of 1.0 are exact, so the entry is log of the correctly rounded 1 / S)."""
    assert np.all(lp == lp[0, 0]) and lp[0, 0] == inf["logp1_unseen"]
    assert abs(lp[0, 0] + math.log(inf["S"])) <= 1e-12


# ── the first verify pass, from the Python restatement ──────────────────────

@functools.lru_cache(maxsize=None)
def _tables(code):
    m, k, n, taps = CODES[code]
    return R.encoder_tables(taps, m, k, n)


@functools.lru_cache(maxsize=None)
def _chain(code, p, seed, L):
    """(received words r[0..L), [D_0 .. D_L] as tuples) of the learning chain"""
    m, k, n, taps = CODES[code]
    r = R.received_stream(taps, m, k, n, L, p, seed, philox.LEARN_TAG, 0)
    out_sym, nxt = _tables(code)
    D = np.zeros(1 << m, np.int64)
    out = [tuple(D)]
    for t in range(L):
        D = R.metric_step_vec(D, out_sym, nxt, int(r[t]), n)
        out.append(tuple(int(x) for x in D))
    return r, out


def _walk(code, r, t0, t1):
    """D = 0 advanced over steps t0 .. t1"""
    m, k, n, taps = CODES[code]
    out_sym, nxt = _tables(code)
    D = np.zeros(1 << m, np.int64)
    for t in range(t0, t1):
        D = R.metric_step_vec(D, out_sym, nxt, int(r[t]), n)
    return tuple(int(x) for x in D)


@functools.lru_cache(maxsize=None)
def mismatched_blocks(code, p, seed, L, blen, warm):
    """The blocks b >= 1 whose speculative start -- D = 0 advanced over steps
    max(0, b blen - warm) .. b blen -- differs from the true D_{b blen}, as metric vectors (for a
    dense model the BFS indices differ iff the vectors do)."""
    r, true = _chain(code, p, seed, L)
    nblocks = -(-L // blen)
    return tuple(b for b in range(1, nblocks) if _walk(code, r, max(0, b * blen - warm), b * blen) != true[b * blen])


def expected_mismatches(code, p, seed, L, blen, warm):
    return len(mismatched_blocks(code, p, seed, L, blen, warm))


@functools.lru_cache(maxsize=None)
def boundary_mismatches(code, p, seed, L, blen, warm):
    """What the verify pass compares, literally: block b's speculative start against block b - 1's
    speculative END (block b - 1 walked from its own speculative start), not against the truth.
    The two counts can differ only if a block that started wrong ends where its successor's
    shorter warm-up also ends; test_learn_cases_host.py checks that they agree at every geometry
    case, so the exact expectation holds for the kernel as written."""
    r, _ = _chain(code, p, seed, L)
    nblocks = -(-L // blen)
    return sum(_walk(code, r, max(0, b * blen - warm), b * blen)
               != _walk(code, r, max(0, (b - 1) * blen - warm), b * blen) for b in range(1, nblocks))

"""tests/learn_cases.py on the CPU: at every case that test_gpu_learn_edges.py gives the GPU
chain, the product's HOST chain builds the C oracle's model (so the GPU file's reference is the
contract, and a failure there lies in csrc/cvd_learn.hip or the generator that feeds it); and
the block-mismatch simulation has the properties the GPU file relies on."""
import numpy as np
import pytest

import learn_cases as LC
from oracle import c_oracle as C


@pytest.fixture(autouse=True)
def _no_model_cache(monkeypatch):
    monkeypatch.delenv("CVD_MODEL_CACHE", raising=False)


def test_code_table(pkg):
    for name, cfg in (("m2", "m2"), ("m6", "m6"), ("r23", "r23_m4")):
        cc = pkg.CONFIG_CODES[cfg]
        assert LC.CODES[name] == (cc["m"], cc["k"], cc["n"], cc["gen1"])
    for name, (m, k, n, taps) in LC.CODES.items():
        assert len(taps) == n and all(len(row) == k and all(len(t) == m + 1 for t in row) for row in taps), name
    assert len(LC.ALL_CASES) == len(set(LC.ALL_CASES))


@pytest.mark.parametrize("case", LC.ALL_CASES, ids=LC.case_id)
def test_host_chain_equals_c_oracle(pkg, case):
    inf, lp, _ = LC.assert_equals_oracle(pkg, LC.product_model(pkg, case), case)
    assert inf["kind"] == (1 if case.cap == LC.SPARSE_CAP else 0)
    if case.L is not None and case.burn >= case.L:
        LC.assert_laplace_rows(inf, lp)


def test_anchors():
    """the visited-state counts the cases were chosen by (the oracle's, recomputed)"""
    S = {(c, L): LC.oracle_model(LC.Case(c, 0.05, L, 0, LC.SPARSE_CAP)).S for c in LC.SPARSE_CODES
         for L in (1, 2, 257, 3000)}
    assert [S[c, 257] for c in LC.SPARSE_CODES] == [28, 92, 169, 213, 248, 131]
    assert [S[c, 3000] for c in LC.SPARSE_CODES] == [31, 284, 1299, 1957, 2437, 549]
    assert all(S[c, 1] == 2 and S[c, 2] == 3 for c in LC.SPARSE_CODES)
    dense = {c: LC.oracle_model(LC.Case(c, 0.05, None, 200, LC.DENSE_CAP)) for c in LC.DENSE_CODES}
    assert all(om.kind == 0 for om in dense.values())
    assert {c: om.S for c, om in dense.items()} == {"n1": 1, "m2": 31, "m3": 471, "r13": 85, "r23": 1807}
    assert {c: C.lib().oc_model_learn_len(om.h) for c, om in dense.items()} == \
        {"n1": 5000, "m2": 6200, "m3": 94_200, "r13": 17_000, "r23": 361_400}
    # p = 0.2: nearly every step of the long-key codes is a first visit
    for c in ("m5", "m6"):
        assert LC.oracle_model(LC.Case(c, 0.2, 3000, 200, LC.SPARSE_CAP)).S > 0.9 * 3001


SIM_CODES = ["m3", "m4", "m5", "m6", "r13"]


@pytest.mark.parametrize("code", SIM_CODES)
def test_expected_mismatches_quoted_values(code):
    p, seed, L = LC.GEOMETRY_P, LC.SEED, 3000
    assert LC.expected_mismatches(code, p, seed, L, 64, 0) == 46       # every block but block 0
    assert LC.expected_mismatches(code, p, seed, L, 64, 3) == 46
    assert LC.expected_mismatches(code, p, seed, L, 1, 0) == 2999
    assert LC.expected_mismatches(code, p, seed, 2049, 256, 0) == 8
    assert LC.expected_mismatches(code, p, seed, L, 64, 512) == 0
    assert LC.expected_mismatches(code, p, seed, L, 300, 16) == {"m3": 0, "r13": 0, "m4": 4, "m5": 9, "m6": 9}[code]


@pytest.mark.parametrize("code", SIM_CODES)
def test_expected_mismatches_sanity(code):
    p, seed = LC.GEOMETRY_P, LC.SEED
    for L, blen in ((300, 64), (257, 256), (40, 1)):
        assert LC.expected_mismatches(code, p, seed, L, blen, L) == 0           # warm >= L: every start exact
        assert LC.expected_mismatches(code, p, seed, L, blen, L + 7) == 0
    for L in (1, 2, 256):
        assert LC.expected_mismatches(code, p, seed, L, 256, 0) == 0            # a single block
    assert LC.expected_mismatches(code, p, seed, 257, 256, 0) == 1              # D_256 != 0
    bad = LC.mismatched_blocks(code, p, seed, 3000, 300, 16)
    assert list(bad) == sorted(set(bad)) and all(1 <= b < 10 for b in bad)


@pytest.mark.parametrize("case,blen,warm", LC.GEOMETRY_CASES,
                         ids=[f"{c.code}-L{c.L}-b{b}-w{w}" for c, b, w in LC.GEOMETRY_CASES])
def test_verify_pass_counts_what_the_simulation_counts(case, blen, warm):
    """block b's start against block b - 1's speculative end (what verify_kernel compares) gives
    the count of starts that differ from the truth, at every geometry case"""
    args = (case.code, case.p, LC.SEED, case.L, blen, warm)
    assert LC.boundary_mismatches(*args) == LC.expected_mismatches(*args)


@pytest.mark.parametrize("code", LC.SPARSE_CODES)
def test_default_warm_up_leaves_no_mismatch(code):
    for p in (0.05, 0.2):
        assert LC.expected_mismatches(code, p, LC.SEED, 3000, LC.DEFAULT_BLEN, LC.DEFAULT_WARM) == 0

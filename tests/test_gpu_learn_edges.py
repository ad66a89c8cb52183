"""The GPU learning chain (csrc/cvd_learn.hip) at every kernel instance and block edge, against
the C oracle (oracle/cvd_oracle.c), which shares no code with the product; the host chain equals
the oracle at every case here (test_learn_cases_host.py), and every case asserts host_fallback == 0.
Every comparison is exact: kind, S, the keys in first-visit order, log P̂1 bit for bit.

Kernel instances and the cases that launch them (tests/learn_cases.py):

  chain_sparse_kernel<2,1,2>  NW 1   test_sparse_instances[m2-*]
  chain_sparse_kernel<3,1,2>  NW 1   test_sparse_instances[m3-*], test_burn_edges[m3-*], test_block_geometry[m3-*]
  chain_sparse_kernel<4,1,2>  NW 2   test_sparse_instances[m4-*], test_block_geometry[m4-*], test_hash_*
  chain_sparse_kernel<5,1,2>  NW 4   test_sparse_instances[m5-*], test_block_geometry[m5-*]
  chain_sparse_kernel<6,1,2>  NW 8   test_sparse_instances[m6-*]
  chain_sparse_kernel<4,2,3>  NW 2   test_sparse_instances[r23-*]
  chain_dense_kernel<1>              test_dense_instances[n1-*]   (32 steps per word, generic generator)
  chain_dense_kernel<2>              test_dense_instances[m2-*, m3-*]
  chain_dense_kernel<3>              test_dense_instances[r13-*, r23-*], test_burn_edges[r13-*],
                                     test_block_geometry[r13-*]   (r13: 10 steps per word, gen_fast_variant<1,3>)

With NW = 1 hash_kernel's odd-word branch supplies the missing high word, with NW = 2, 4, 8 it
never does; verify / gather / heads / rowkeys run at nw = 1, 2, 4, 8.  Lengths 1 and 2 (a sort
and two scans of 2 and 3 entries), 255 / 256 / 257 and 2048 / 2049 (the last block full, and one
step long: the e0 == L write of states[L]), lengths that are no multiple of the steps per word or
of the stream's 4-word rounding, burn 0 / L - 1 / L / L + 5, block length 1.  The repair
statistics are exact: mismatched_blocks is the count that the Python restatement predicts
(learn_cases.expected_mismatches), the sequential tail starts at the first failing block.  The
hash-collision retry runs through CVD_LEARN_HASH_BITS / CVD_LEARN_HASH_WEAK."""
import pytest
import torch

import learn_cases as LC

pytestmark = pytest.mark.gpu

KNOBS = ("CVD_LEARN_BLOCK", "CVD_LEARN_WARM", "CVD_LEARN_MAX_PASSES", "CVD_LEARN_HASH_BITS", "CVD_LEARN_HASH_WEAK",
         "CVD_GEN_FORM", "CVD_GEN_TAP_LOOP", "CVD_GEN_GENERIC", "CVD_GEN_SLOTS")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    """no model cache (the knobs are not part of its key) and no knob left over"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    monkeypatch.delenv("CVD_MODEL_CACHE", raising=False)
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)


def _gpu(pkg, case):
    """the GPU chain's model of `case`, equal to the C oracle's, not built by the host fallback"""
    model = LC.product_model(pkg, case, learn_device=0)
    st = model.learn_stats
    print(f"\n  {LC.case_id(case)}: S={model.info()['S']} stats {st}")
    assert st["host_fallback"] == 0, st
    inf, lp, _ = LC.assert_equals_oracle(pkg, model, case)
    assert st["hash_attempts"] == (1 if inf["kind"] == 1 else 0), st
    return model, inf, lp


def _default_geometry_mismatches(case):
    """default block length and warm-up; a block whose warm-up reaches back to step 0 starts exact
    (L <= 768), else the simulation"""
    if case.L <= LC.DEFAULT_BLEN + LC.DEFAULT_WARM:
        return 0
    return LC.expected_mismatches(case.code, case.p, LC.SEED, case.L, LC.DEFAULT_BLEN, LC.DEFAULT_WARM)


@pytest.mark.parametrize("case", LC.SPARSE_CASES, ids=LC.case_id)
def test_sparse_instances(pkg, case):
    model, inf, _ = _gpu(pkg, case)
    assert inf["kind"] == 1
    want = _default_geometry_mismatches(case)
    assert want == 0 and model.learn_stats["mismatched_blocks"] == 0 == model.learn_stats["fix_passes"]


@pytest.mark.parametrize("case", LC.DENSE_CASES, ids=LC.case_id)
def test_dense_instances(pkg, case):
    model, inf, _ = _gpu(pkg, case)
    assert inf["kind"] == 0
    if case.L is not None:
        assert model.learn_stats["mismatched_blocks"] == _default_geometry_mismatches(case) == 0


@pytest.mark.parametrize("case", LC.BURN_CASES, ids=LC.case_id)
def test_burn_edges(pkg, case):
    _, inf, lp = _gpu(pkg, case)
    if case.burn >= case.L:
        LC.assert_laplace_rows(inf, lp)
    else:
        assert not (lp == lp[0, 0]).all()       # burn = L - 1: the one counted step shows


GEOMETRY_RUNS = [(c, b, w, mp) for c, b, w in LC.GEOMETRY_CASES for mp in ((None, "0", "1") if b == 1 else (None, "0"))]


@pytest.mark.parametrize("case,blen,warm,max_passes", GEOMETRY_RUNS,
                         ids=[f"{c.code}-L{c.L}-b{b}-w{w}-passes{mp}" for c, b, w, mp in GEOMETRY_RUNS])
def test_block_geometry(pkg, monkeypatch, case, blen, warm, max_passes):
    """speculative blocks that start wrong are counted exactly and repaired, by the parallel passes
    and by the sequential tail"""
    monkeypatch.setenv("CVD_LEARN_BLOCK", str(blen))
    monkeypatch.setenv("CVD_LEARN_WARM", str(warm))
    if max_passes is not None:
        monkeypatch.setenv("CVD_LEARN_MAX_PASSES", max_passes)
    bad = LC.mismatched_blocks(case.code, case.p, LC.SEED, case.L, blen, warm)
    nblocks = -(-case.L // blen)
    model, _, _ = _gpu(pkg, case)
    st = model.learn_stats
    assert st["mismatched_blocks"] == len(bad) == LC.expected_mismatches(case.code, case.p, LC.SEED, case.L, blen, warm)
    if not bad:
        assert st["fix_passes"] == 0 and st["sequential_blocks"] == 0
    elif max_passes == "0":
        assert st["fix_passes"] == 0 and st["sequential_blocks"] == nblocks - bad[0]
    elif max_passes == "1":
        # one parallel pass makes (at least) the first failing block exact; the tail starts later
        assert st["fix_passes"] == 1 and 0 < st["sequential_blocks"] < nblocks - bad[0]
    else:
        assert 1 <= st["fix_passes"] <= 8
        assert st["sequential_blocks"] == 0 or st["fix_passes"] == 8


def test_hash_collision_retry(pkg, monkeypatch):
    """3 hash bits on the first attempt: 1299 keys in at most 8 hash values collide for certain;
    the second attempt (another seed, all 64 bits, the collision flag cleared) gives the model.
    (The re-zeroing of isfirst cannot be observed: the sort is stable in t, so the head of a
    segment of equal hashes is the smallest t with that hash, which is the first visit of its key
    whatever the hash; a failed attempt only ever marks true first visits.)"""
    monkeypatch.setenv("CVD_LEARN_HASH_BITS", "3")
    model = LC.product_model(pkg, LC.COLLISION_CASE, learn_device=0)
    assert model.learn_stats["host_fallback"] == 0 and model.learn_stats["hash_attempts"] == 2, model.learn_stats
    inf, _, _ = LC.assert_equals_oracle(pkg, model, LC.COLLISION_CASE)
    assert inf["S"] == 1299


def test_hash_collision_retry_twice(pkg, monkeypatch):
    """CVD_LEARN_HASH_WEAK = 2: two narrowed attempts fail, the third gives the model"""
    monkeypatch.setenv("CVD_LEARN_HASH_BITS", "3")
    monkeypatch.setenv("CVD_LEARN_HASH_WEAK", "2")
    model = LC.product_model(pkg, LC.COLLISION_CASE, learn_device=0)
    assert model.learn_stats["host_fallback"] == 0 and model.learn_stats["hash_attempts"] == 3, model.learn_stats
    LC.assert_equals_oracle(pkg, model, LC.COLLISION_CASE)


def test_persistent_hash_collisions_are_an_error(pkg, monkeypatch):
    """all four attempts narrowed: CVD_E_STATE with the collisions named -- no model, and no host
    fallback (which would return one)"""
    monkeypatch.setenv("CVD_LEARN_HASH_BITS", "3")
    monkeypatch.setenv("CVD_LEARN_HASH_WEAK", "4")
    with pytest.raises(pkg.CvdError, match="libcvd error -5: .*hash collisions"):
        LC.product_model(pkg, LC.COLLISION_CASE, learn_device=0)
    monkeypatch.delenv("CVD_LEARN_HASH_BITS")
    _gpu(pkg, LC.COLLISION_CASE)                 # the next model of the process is unaffected


def test_wide_narrowed_hash_does_not_collide(pkg, monkeypatch):
    """40 bits: 1299 keys collide with probability 8e-7; one attempt"""
    monkeypatch.setenv("CVD_LEARN_HASH_BITS", "40")
    model = LC.product_model(pkg, LC.COLLISION_CASE, learn_device=0)
    assert model.learn_stats["host_fallback"] == 0 and model.learn_stats["hash_attempts"] == 1, model.learn_stats
    LC.assert_equals_oracle(pkg, model, LC.COLLISION_CASE)

"""The T_ref count behind the one-plane test in the m = 6 detector k1s (csrc/cvd_bitslice.h
CVD_BS_TREF_FAST, csrc/cvd_k1s.h bs_lt_add): most wave-steps take c = 1 for all their lanes
and add the constant ltref[1]; a wave-step with a suspect lane runs the exact count.  The
per-sequence sums (log P̂1, log T_ref) must stay bit-identical to the C oracle's and the counts
equal -- through the lockstep loop, walk mode, a chunked launch (counts: a chunked launch
returns no sums) and detect_multi -- and identical to the knob-off build's, which counts
exactly in every lane at every step.

Shape: the m = 6 pair, N = 768 (128 six-step groups), 256 trials = 512 sequences, so every
wave is all-H1 or all-H2; step 0 alone, from D_0 = 0, has c > 1 (c = 2) in every sequence (the
exact path with a count above 1).  Of the 3 * 512 * 767 later steps the oracle counts c > 1 at
one (p = 0.2, an H2 sequence; tests/test_oracle_score_host.py asserts it): there the exact path is entered only for suspects whose count
turns out to be 1, and the g1 = g2 (kUni, c = 4) instantiations never run here
(tests/test_gpu_foreign_streams.py has both).  p = 0.01 / 0.05 / 0.2: the LDS-filter, the
pre-filter and the plain-filter variants of the kernel."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

SEED = 12345
N, T, LEARN = 768, 256, 300_000
PS = [0.01, 0.05, 0.2]


class _Point:
    def __init__(self, pkg, det, cc, p):
        self.p = p
        self.model = det.model(p, LEARN, 200, 1.0, SEED)
        g1, g2 = pkg.Code(cc["gen1"], 6, 1, 2), pkg.Code(cc["gen2"], 6, 1, 2)
        tag = pkg.grid_tag(N, p)
        self.r = det.stream_buffer(N, 2 * T)
        det.generate(g1, N, p, SEED, tag, 0, 2, T, out=self.r, q0=0, pitch=2 * T)
        det.generate(g2, N, p, SEED, tag, 1, 2, T, out=self.r, q0=T, pitch=2 * T)
        c1, c2 = C.Code(cc["gen1"], 6, 1, 2), C.Code(cc["gen2"], 6, 1, 2)
        cnt, s = C.Model(c1, p, LEARN, 200, 1.0, SEED).run_trials(c1, c2, N, p, SEED, 0, T, sums=True, nthreads=16)
        self.counts = [int(x) for x in cnt]
        self.sums = np.concatenate([s[:, :2], s[:, 2:]])   # detect's order: the H1 sequences, then the H2
        self.sums.setflags(write=False)


@pytest.fixture(scope="module")
def m6(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cc = pkg.CONFIG_CODES["m6"]
    det = pkg.Detector(1, 2, 6, cc["gen1"], device=0)
    return cc, det, {p: _Point(pkg, det, cc, p) for p in PS}


def _detect(det, model, r):
    s = torch.empty((2 * T, 2), dtype=torch.float64, device=det.device)
    c = det.detect(model, r, N, 2 * T, T, sums=s)
    torch.cuda.synchronize()
    assert model.device_error() == 0
    return s.cpu().numpy(), c.cpu().tolist()


@pytest.mark.parametrize("p", PS)
def test_lockstep_sums_equal_c_oracle(pkg, m6, monkeypatch, p):
    cc, det, pts = m6
    pt = pts[p]
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_CHUNK", "0")
    got, cnt = _detect(det, pt.model, pt.r)
    inf = pt.model.info()
    print("p", p, "kernel", pkg.KERNEL_NAMES[inf["explicit_kernel"]], "lds_filter", inf["lds_filter"])
    assert "bit-sliced" in pkg.KERNEL_NAMES[inf["explicit_kernel"]], inf
    assert np.array_equal(got, pt.sums)
    assert cnt == pt.counts


@pytest.mark.parametrize("p", PS)
def test_walk_mode_sums_equal_c_oracle(pkg, m6, monkeypatch, p):
    cc, det, pts = m6
    pt = pts[p]
    monkeypatch.setenv("CVD_WALK", "1")
    monkeypatch.setenv("CVD_CHUNK", "0")
    got, cnt = _detect(det, pt.model, pt.r)
    assert np.array_equal(got, pt.sums)
    assert cnt == pt.counts


@pytest.mark.parametrize("p", PS)
def test_chunked_launch_counts_equal_c_oracle(pkg, m6, monkeypatch, p):
    cc, det, pts = m6
    pt = pts[p]
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "192")
    c = det.detect(pt.model, pt.r, N, 2 * T, T)
    torch.cuda.synchronize()
    st = pkg._lib.chunk_last()
    assert st["groups"] == 1 and st["C"] >= 2, st
    assert c.cpu().tolist() == pt.counts, st
    assert pt.model.device_error() == 0


def test_detect_multi_sums_equal_c_oracle(pkg, m6, monkeypatch):
    cc, det, pts = m6
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_CHUNK", "0")
    cnts = [torch.zeros(2, dtype=torch.int64, device=det.device) for _ in PS]
    sums = [torch.empty((2 * T, 2), dtype=torch.float64, device=det.device) for _ in PS]
    det.detect_multi([pts[p].model for p in PS], [pts[p].r for p in PS], N, [2 * T] * len(PS), [T] * len(PS), cnts,
                     sums=sums)
    torch.cuda.synchronize()
    for p, c, s in zip(PS, cnts, sums):
        assert np.array_equal(s.cpu().numpy(), pts[p].sums), p
        assert c.cpu().tolist() == pts[p].counts, p
        assert pts[p].model.device_error() == 0


def test_knob_off_build_bit_identical(pkg, m6, monkeypatch):
    """-DCVD_BS_TREF_FAST=0 (the exact count in every lane at every step) through
    CVD_JIT_DEFINES: the same sums as the default build on the same streams"""
    cc, det, pts = m6
    pt = pts[0.05]
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_CHUNK", "0")
    ref, rc = _detect(det, pt.model, pt.r)
    monkeypatch.setenv("CVD_JIT_DEFINES", "-DCVD_BS_TREF_FAST=0")
    off = pkg.Model(det.dec, pt.p, LEARN, 200, 1.0, SEED).upload(0)
    monkeypatch.delenv("CVD_JIT_DEFINES")
    assert off.jit_status()[0] == 1, off.jit_status()
    got, gc = _detect(det, off, pt.r)
    assert np.array_equal(got, ref)
    assert np.array_equal(got, pt.sums)
    assert gc == rc == pt.counts

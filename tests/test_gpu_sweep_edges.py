"""cvd_parity_sweep (csrc/cvd_sweep.hip) at every kernel instance, every B and the edges of its
tile loop, against tests/sweep_cases.py's reference, which test_sweep_cases_host.py pins to the
definition (count the anchors whose masked word has even parity).  Every comparison is of the
whole [n_phase, 2^B] array, for exact equality.

  sweep_hist_kernel<n, format, mode>   all 27: whole LDS at B <= 15, LDS parts at 16..21, global
                                       atomics natively at B = 22 (n = 1, 2) and through
                                       CVD_SWEEP_GLOBAL_B = 16 at B = 18 (n = 3 has no B = 22)
  sweep_wht_kernel                     every B = 1..22 (n = 1)
  the tile loop                        blocks that take a second and a third tile in LDS-parts,
                                       whole-LDS and global mode, beside a control that does not
  capture and tile edges               start mod 128 = 0, 1, 127 and a start past the first tile;
                                       a last word that begins on a tile's last bit / on the next
                                       tile's first bit; a capture that ends on a piece and on a
                                       tile (the overlap piece wholly past the capture), with a
                                       piece of ones allocated behind it; T = 1 and 2
  structured histograms                all ones and 0101... at B = 13, 16, 19, 22
  the i32 edge                         2^31 - 1 anchors in one bin

No case sets anything but CVD_SWEEP_GLOBAL_B."""
import time

import numpy as np
import pytest
import torch

import sweep_cases as SC
from test_gpu_capture import capture_bits, raw_capture

pytestmark = pytest.mark.gpu

KNOB = "CVD_SWEEP_GLOBAL_B"


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    """no knob left over"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    monkeypatch.delenv(KNOB, raising=False)


def _raw(c, bits):
    """The capture's buffer: every bit of it past the capture's last bit is a one (a reading past
    nbits that reached a word would change a count).  pad: a capture that may end on a piece gets
    a further piece of ones behind it, as raw_capture pads the others."""
    rng = np.random.default_rng(1)
    nbits = len(bits)
    raw = raw_capture(np.concatenate([bits, np.ones(128, np.uint8)]) if c.pad else bits, c.fmt, rng)
    every = capture_bits(raw, c.fmt, len(raw) if c.fmt == "bytes" else 8 * len(raw))
    assert np.array_equal(every[:nbits], bits) and every[nbits:].all() and len(raw) % 16 == 0
    assert c.pad == (nbits % 128 == 0) and (not c.pad or len(every) >= nbits + 128)
    return raw


def _sweep(pkg, c, raw, nbits):
    got = pkg.parity_sweep(raw, c.n, c.span, start=c.start, T=c.T, n_phase=c.n_phase, format=c.fmt, nbits=nbits)
    assert got.dtype == torch.int64 and tuple(got.shape) == (c.n_phase, 1 << SC.word_bits(c))
    return got.cpu().numpy()


def _check(pkg, monkeypatch, c):
    """the case through the kernels, equal to the reference everywhere; returns (got, raw, nbits)"""
    bits = SC.case_bits(c)
    raw = _raw(c, bits)
    want = SC.case_reference(c, bits)
    if c.global_b is not None:
        monkeypatch.setenv(KNOB, str(c.global_b))
    got = _sweep(pkg, c, raw, len(bits))
    monkeypatch.delenv(KNOB, raising=False)
    wrong = got != want
    assert not wrong.any(), (SC.sweep_id(c), int(wrong.sum()), np.argwhere(wrong)[:4].tolist(),
                             got[wrong][:4].tolist(), want[wrong][:4].tolist())
    assert np.all(want[:, 0] == c.T)
    return got, raw, len(bits)


@pytest.mark.parametrize("c", SC.INSTANCE_CASES, ids=SC.sweep_id)
def test_every_histogram_instance(pkg, monkeypatch, c):
    got, raw, nbits = _check(pkg, monkeypatch, c)
    if c.global_b is not None:
        # the variable is read on every call: without it the same shape runs in LDS parts
        assert SC.instance_of(c.n, c.span, c.fmt) != SC.instance_of(c.n, c.span, c.fmt, c.global_b)
        assert np.array_equal(_sweep(pkg, c, raw, nbits), got)


@pytest.mark.parametrize("c", SC.WHT_CASES, ids=SC.sweep_id)
def test_every_B(pkg, monkeypatch, c):
    _check(pkg, monkeypatch, c)


@pytest.mark.parametrize("c", [c for c, _ in SC.STRIDE_CASES], ids=SC.sweep_id)
def test_grid_stride(pkg, monkeypatch, c):
    """ntiles > gx (test_sweep_cases_host.py): a block stages a second and a third tile behind
    the barrier while its LDS histogram persists; the third case is the control, gx = ntiles"""
    _check(pkg, monkeypatch, c)


@pytest.mark.parametrize("c", [c for _, c in SC.ALIGN_CASES],
                         ids=[end + "_" + SC.sweep_id(c) for end, c in SC.ALIGN_CASES])
def test_alignment(pkg, monkeypatch, c):
    _check(pkg, monkeypatch, c)


@pytest.mark.parametrize("c", SC.TINY_CASES, ids=SC.sweep_id)
def test_one_and_two_anchors(pkg, monkeypatch, c):
    _check(pkg, monkeypatch, c)


@pytest.mark.parametrize("c", SC.STRUCTURED_CASES, ids=SC.sweep_id)
def test_structured_histograms(pkg, monkeypatch, c):
    """one bin (all ones) or two (0101...) hold every anchor: every sign of the transform matters"""
    got, _, _ = _check(pkg, monkeypatch, c)
    if c.fill == "ones":
        assert np.array_equal(got, SC.constant_sat(1, SC.word_bits(c), c.T, c.n_phase))


@pytest.mark.parametrize("value", [1, 0])
def test_2_31_anchors_in_one_bin(pkg, value):
    """The i32 exactness argument at its edge: T = 2^31 - 1 anchors, all in one bin of the LDS
    histograms, so the transform's partial sums reach +-(2^31 - 1).  A constant LSB capture of
    2^31 + 128 bits made on the device; the expected array is constant_sat's closed form, which
    test_sweep_cases_host.py checks against the reference at T = 70,001.  Measured on an MI355X:
    either sweep (2^31 - 1 LDS atomics on one address per block) takes 7 ms."""
    c = SC.I32_CASE
    cap = torch.full((SC.I32_NBITS // 8,), 0xFF if value else 0, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = pkg.parity_sweep(cap, c.n, c.span, start=c.start, T=c.T, format=c.fmt, nbits=SC.I32_NBITS)
    torch.cuda.synchronize()
    print(f"\nsweep of {c.T} anchors in one bin (value {value}): {time.perf_counter() - t0:.3f} s")
    assert np.array_equal(got.cpu().numpy(), SC.constant_sat(value, SC.word_bits(c), c.T, 1))

"""The two forms of the k = 1, n = 2 generator (csrc/cvd_kernels.hip gen_fast_kernel<1, 2, kT, kVK>:
the noise keys' round keys in VGPRs, 80 registers, or as scalar operands, <= 64, the form whose
waves fit beside the m = 6 detector's; CVD_GEN_FORM=fast / small forces one) must write
identical words, equal to the oracle's stream.

N = 773 is 49 stream words: a partial last 16-byte chunk.  65 and 257 sequences: a partial wave
and a partial block.  Both codes of the m = 6 pair, p from 0.0033 (nearly every noise plane
decided in the head) to 0.2."""
import numpy as np
import pytest
import torch

from oracle import philox
from oracle import restatement as R

pytestmark = pytest.mark.gpu
SEED = 0x5EED_1234


def _unpack(words, n, N):
    b = words.cpu().numpy().view(np.uint32).astype(np.int64)
    w = b.transpose(0, 2, 1).reshape(-1, b.shape[1])
    spw = 32 // n
    t = np.arange(N)
    return (w[t // spw, :] >> ((t % spw) * n)[:, None]) & ((1 << n) - 1)


@pytest.fixture(scope="module")
def det(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cc = pkg.CONFIG_CODES["m6"]
    return cc, pkg.Detector(1, 2, 6, cc["gen1"], device=0)


def _both(det, taps, N, p, base, stride, count, monkeypatch):
    tag = philox.grid_tag(N, p)
    out = {}
    for form in ("fast", "small"):
        monkeypatch.setenv("CVD_GEN_FORM", form)
        out[form] = det.generate(taps, N, p, SEED, tag, base, stride, count)
    monkeypatch.delenv("CVD_GEN_FORM")
    torch.cuda.synchronize()
    return tag, out["fast"], out["small"]


@pytest.mark.parametrize("count", [65, 257])
@pytest.mark.parametrize("p", [0.0033, 0.01, 0.2])
@pytest.mark.parametrize("gen", ["gen1", "gen2"])
def test_forms_agree_and_equal_oracle(det, monkeypatch, gen, p, count):
    cc, d = det
    taps, N, base, stride = cc[gen], 773, 11, 2
    assert d.words_per_seq(N) == 52 and -(-N // 16) == 49
    tag, fast, small = _both(d, taps, N, p, base, stride, count, monkeypatch)
    assert torch.equal(fast, small)
    got = _unpack(small, 2, N)
    for q in (0, 63, 64, count - 1):
        want = R.received_stream(taps, 6, 1, 2, N, p, SEED, tag, base + q * stride)
        np.testing.assert_array_equal(got[:, q], want)
    # the padding words of the last chunk stay zero
    assert int(small.cpu().numpy().view(np.uint32)[-1, :, 1:].max()) == 0


@pytest.mark.parametrize("slots", [3, 17])
def test_forms_agree_over_several_exchange_rounds(det, monkeypatch, slots):
    """CVD_GEN_SLOTS below 64 (GenArgs::slots): the stragglers of a chunk take several rounds"""
    cc, d = det
    taps, N, p, count = cc["gen1"], 4099, 0.2, 200
    tag, ref, _ = _both(d, taps, N, p, 3, 1, count, monkeypatch)
    monkeypatch.setenv("CVD_GEN_SLOTS", str(slots))
    _, fast, small = _both(d, taps, N, p, 3, 1, count, monkeypatch)
    monkeypatch.delenv("CVD_GEN_SLOTS")
    assert torch.equal(fast, ref) and torch.equal(small, ref)
    got = _unpack(small, 2, N)
    for q in (0, 77, count - 1):
        np.testing.assert_array_equal(got[:, q], R.received_stream(taps, 6, 1, 2, N, p, SEED, tag, 3 + q))

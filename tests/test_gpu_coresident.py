"""The next batch's generator beside a persistent m = 6 detector launch, as bench.py's overlap path
issues them: the detector (k1s through its work queue, a batch just past
cvd_model_info.persist_seqs) on one stream, the two generator launches (H1 then H2 code) on a
second one.  The library then takes the small generator form, whose waves fit on the SIMDs the
detector's waves occupy (csrc/cvd_kernels.hip gen_small_form).  Counts, per-sequence sums and the
generated words must equal the same work done serially, with the fast generator form.

N = 192 (12 stream words, three whole chunks, 32 six-step groups) keeps the launch over the
262,272 sequences short.  p = 0.01: the LDS-filter variant of the kernel; p = 0.1: the
pre-filter variant."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 12345
N, LEARN = 192, 300_000


@pytest.fixture(scope="module")
def m6(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cc = pkg.CONFIG_CODES["m6"]
    return cc, pkg.Detector(1, 2, 6, cc["gen1"], device=0)


def _gen(pkg, det, cc, p, tb, B, buf, stream=None):
    g1, g2 = pkg.Code(cc["gen1"], 6, 1, 2), pkg.Code(cc["gen2"], 6, 1, 2)
    tag = pkg.grid_tag(N, p)
    det.generate(g1, N, p, SEED, tag, 2 * tb, 2, B, out=buf, q0=0, pitch=2 * B, stream=stream)
    det.generate(g2, N, p, SEED, tag, 2 * tb + 1, 2, B, out=buf, q0=B, pitch=2 * B, stream=stream)


@pytest.mark.parametrize("p,ldsf", [(0.01, 1), (0.1, 0)])
def test_generator_beside_persistent_detector(pkg, m6, monkeypatch, p, ldsf):
    cc, det = m6
    for v in ("CVD_WALK", "CVD_GEN_FORM", "CVD_K1S_PERSIST", "CVD_K1S_PERSIST_BLOCKS"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("CVD_CHUNK", "0")
    model = det.model(p, LEARN, 200, 1.0, SEED)
    inf = model.info()
    assert "bit-sliced" in pkg.KERNEL_NAMES[inf["explicit_kernel"]] and inf["lds_filter"] == ldsf, inf
    cap = inf["persist_seqs"]
    assert cap > 0, inf
    B = cap // 2 + 64
    nseq = 2 * B
    assert cap < nseq <= cap + 128
    dev = det.device

    # serially, on the current stream, the fast generator form
    monkeypatch.setenv("CVD_GEN_FORM", "fast")
    buf_a, buf_b = det.stream_buffer(N, nseq), det.stream_buffer(N, nseq)
    _gen(pkg, det, cc, p, 0, B, buf_a)
    torch.cuda.synchronize()
    sums = torch.empty((nseq, 2), dtype=torch.float64, device=dev)
    counts = det.detect(model, buf_a, N, nseq, B, sums=sums)
    torch.cuda.synchronize()
    _gen(pkg, det, cc, p, B, B, buf_b)
    torch.cuda.synchronize()
    monkeypatch.delenv("CVD_GEN_FORM")
    assert model.device_error() == 0

    # the detector on the main stream, the next batch's generator on a second one (default rule)
    main, gstream = torch.cuda.current_stream(), torch.cuda.Stream(device=dev)
    buf_b2 = torch.zeros_like(buf_b)
    sums2 = torch.empty_like(sums)
    counts2 = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    det.detect(model, buf_a, N, nseq, B, sums=sums2, counts=counts2, stream=main)
    _gen(pkg, det, cc, p, B, B, buf_b2, stream=gstream)
    main.wait_stream(gstream)
    torch.cuda.synchronize()
    assert model.device_error() == 0
    print("p", p, "persist_seqs", cap, "nseq", nseq, "counts", counts.tolist())
    assert counts2.tolist() == counts.tolist()
    assert torch.equal(sums2, sums)
    assert torch.equal(buf_b2, buf_b)

    # and with the small form forced while nothing runs beside it
    monkeypatch.setenv("CVD_GEN_FORM", "small")
    buf_b3 = torch.zeros_like(buf_b)
    _gen(pkg, det, cc, p, B, B, buf_b3)
    torch.cuda.synchronize()
    assert torch.equal(buf_b3, buf_b)

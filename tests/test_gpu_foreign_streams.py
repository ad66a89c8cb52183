"""The m = 6 detector (the bit-sliced k1s behind cvd_detect, its nibble-packed sibling, walk
mode, the chunked launch, detect_multi, Detector.scan) on decoders other than (133,171) and
on streams that the model's generator never makes, against oracle.c_oracle's score_words:
the per-sequence sums (log P̂1, log T_ref) bit for bit, and the counts.

Detector.scan runs every capture window as an H1 lane (n_h1 = nseq; in walk mode a walking
lane) whatever it holds.  Such lanes leave the learned rows and re-enter them many times: the
slot transitions of BsCursor::resolve / hash_ahead, the directory probe loop, walk mode's
rebuild from the row key, while other lanes of the wave keep walking.

Shape: N = 773 = 6 * 128 + 5 (ragged in the six-phase loop and in the 16-step word), 13 kinds
x 12 replicas = 156 sequences, kind-minor (sequence q has kind q % 13): every 64-lane wave
mixes all kinds and the third wave is partial.  Kinds: tests/foreign_streams.py.

The work-queue launch needs more sequences than two blocks hold: the 156 tiled 14 times.

Models (learn_len 300,000, burn 200, laplace 1, seed 12345): (133,171) at p = 0.01 / 0.05 /
0.2 (the LDS-filter, pre-filter and plain-filter kernels); (171,133) and (135,163) (other
specialisations of the bit-sliced kernel); (133,65), whose g2 has tap 0 clear (no standard
butterfly: a fallback explicit kernel); (133,133) with enum_cap = 0 (g1 = g2, the kUni
instantiations: the one row D = 0, c = 4 at every step).

What the inputs exercise is asserted on the oracle's stats before anything runs on the GPU
(foreign_streams.check_inputs).  Measured totals over the 12 replicas (CPU, the oracle),
share of steps in a learned row / re-entries:
  (133,171) p = 0.01: h1 0.937/87, h2 0.003/1, clean 0.970/13, noisy3x 0.730/321, zeros and
    ones 0.969/12, alt 0.003/12, random 0.003/3, phase1 0.004/6, splice 0.660/87, burst
    0.862/89, inverted 0.930/98, othercode 0.004/3
  (133,171) p = 0.05: h1 0.663/362, h2 0.008/25, clean 0.970/13, noisy3x 0.025/67, zeros and
    ones 0.969/12, alt 0.003/12, random 0.006/21, phase1 0.004/12, splice 0.449/318, burst
    0.597/341, inverted 0.635/423, othercode 0.005/12
  (133,171) p = 0.2: every kind <= 0.016 (clean; the others <= 0.008)
  (171,133), (135,163) at 0.05: as (133,171) within 0.02 of the shares; noisy3x 78 and 89
    re-entries, splice 325 and 344, burst 372 and 380; othercode of (135,163) is its own code
  (133,65) at 0.05: clean 0.979/13, zeros 0.978/24, alt 0.978/12, ones 0.001/0, inverted
    0.003/4, noisy3x 0.033/82, splice 0.448/313, burst 0.613/321, random and phase1 0.004.
    Its g2 has an even number of taps, so the all-ones input encodes to word 1, not 3: for
    this decoder `alt` is the constant codeword (asserted >= 0.9) and `ones` the foreign
    constant (asserted <= 0.05) -- the two kinds trade the classes they have elsewhere.
  (133,133): every D_t is the one row; c = 4 at all 773 steps.
T_ref count: c = 2 at step 0 of every sequence of a non-degenerate decoder.  Past step 0 the
oracle (and a numpy restatement) finds c = 2 at exactly two steps of the 6 * 156 * 773 here:
(133,171) p = 0.01, sequence 14 (h2), t = 356, and (135,163), sequence 131 (h2), t = 581.  So
c > 1 in mid-stream is rare, not absent; these two steps put the exact-count branch of
bs_tref_count with a count above 1 under the comparison.  check_inputs bounds the total per
model by twice the measured one (<= 2) and requires the two known steps."""
import concurrent.futures

import numpy as np
import pytest
import torch

import foreign_streams as F

pytestmark = pytest.mark.gpu

SEED = F.SEED
N, REPL, LEARN, NK, NSEQ = F.N, F.REPL, F.LEARN, F.NK, F.NSEQ
JUNK = 13
MAIN, MODELS, IDS = F.MAIN, F.MODELS, F.IDS
BITSLICED = IDS[:5]          # the decoder/p pairs that must run the bit-sliced kernel


TILE = 14                    # 14 * 156 = 2,184 sequences: more than two blocks of the largest launch (1,024)


class _Point:
    def __init__(self, mid, dec, p):
        self.mid, self.dec, self.p = mid, dec, p
        self.om, self.words, self.want, self.stats = F.reference(dec, p)

    def upload(self, pkg):
        d = self.dec
        self.det = pkg.Detector(1, 2, 6, F.gens(d), device=0, enum_cap=0 if d[0] == d[1] else 500_000)
        self.model = self.det.model(self.p, LEARN, 200, 1.0, SEED)
        self.r = torch.from_numpy(F.pack_layout(self.words).view(np.int32)).cuda()

    def tiled(self):
        """(buffer, reference sums) of the 156 sequences TILE times over: sequence q is
        sequence q % 156, so still of kind q % 13."""
        return self.r.repeat(1, TILE, 1).contiguous(), np.tile(self.want, (TILE, 1))


def counts_of(want, n_h1):
    lp, lr = want.T
    return [int((lp > lr)[:n_h1].sum()), int((lp <= lr)[n_h1:].sum())]


@pytest.fixture(scope="module")
def pts(pkg):
    """The seven oracle models (built once, four at a time on host threads: the C calls
    release the GIL), their words, reference sums and stats; the inputs' conditions; then the
    GPU side."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        out = dict(zip(IDS, ex.map(lambda a: _Point(*a), [(i, d, p) for i, (d, p) in zip(IDS, MODELS)])))
    for mid, pt in out.items():
        F.check_inputs(mid, pt.dec, pt.p, pt.stats)
    for pt in out.values():
        pt.upload(pkg)
    return out


def _mismatch(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return "sequences %s (kinds %s)" % (bad.tolist(), sorted({F.KINDS[q % NK] for q in bad}))


def _check(pt, n_h1, leg, model=None, r=None, want=None):
    """detect over r (default: the point's 156 sequences) against want, sums and counts."""
    model = pt.model if model is None else model
    r, want = (pt.r, pt.want) if r is None else (r, want)
    nseq = len(want)
    s = torch.full((nseq, 2), float("nan"), dtype=torch.float64, device=pt.det.device)
    c = pt.det.detect(model, r, N, nseq, n_h1, sums=s)
    torch.cuda.synchronize()
    assert model.device_error() == 0
    got = s.cpu().numpy()
    assert np.array_equal(got, want), (pt.mid, leg, n_h1, _mismatch(got, want))
    assert c.cpu().tolist() == counts_of(want, n_h1), (pt.mid, leg, n_h1)


@pytest.mark.parametrize("mid", IDS)
def test_detect_equals_score_words(pkg, pts, monkeypatch, mid):
    """n_h1 = nseq (scan's call) and n_h1 = 64 (one H1 wave, then H2 waves).  The (133,171)
    models: CVD_WALK 0 / 1 with the work-queue launch off; the others: the default launch and
    walk mode.  (156 sequences fit one block, so none of these is a work-queue launch:
    test_work_queue_launch.)"""
    pt = pts[mid]
    inf = pt.model.info()
    print(mid, "kernel", pkg.KERNEL_NAMES[inf["explicit_kernel"]], "lds_filter", inf["lds_filter"], "walk",
          inf["walk"], "rows", inf["n_rows"])
    assert inf["n_rows"] == pt.om.S
    if mid in BITSLICED:
        assert "bit-sliced" in pkg.KERNEL_NAMES[inf["explicit_kernel"]], inf
    monkeypatch.setenv("CVD_CHUNK", "0")
    if pt.dec == MAIN:
        legs = [{"CVD_WALK": w, "CVD_K1S_PERSIST": "0"} for w in "01"]
    else:
        legs = [{}, {"CVD_WALK": "1"}]
    for leg in legs:
        for k, v in leg.items():
            monkeypatch.setenv(k, v)
        for n_h1 in (NSEQ, 64):
            _check(pt, n_h1, leg)
        for k in leg:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("mid", IDS[:3])
def test_work_queue_launch(pkg, pts, monkeypatch, mid):
    """CVD_K1S_PERSIST=1 capped at two blocks.  A launch goes through the queue only when its
    sequences need more blocks than that (persist_seqs < nseq), which 156 sequences never do:
    the buffer is the 156 sequences 14 times over (2,184, kind-minor as before, the last wave
    partial), the reference tiled the same way.  Lockstep and walk mode; n_h1 = nseq, and
    n_h1 = 1,000 (a wave that holds H1 and H2 lanes)."""
    pt = pts[mid]
    r, want = pt.tiled()
    nseq = len(want)
    assert nseq == TILE * NSEQ and r.shape[1] == nseq
    monkeypatch.setenv("CVD_CHUNK", "0")
    monkeypatch.setenv("CVD_K1S_PERSIST", "1")
    monkeypatch.setenv("CVD_K1S_PERSIST_BLOCKS", "2")
    cap = pt.model.info()["persist_seqs"]
    print(mid, "persist_seqs", cap, "nseq", nseq)
    assert 0 < cap < nseq, cap
    for walk in "01":
        monkeypatch.setenv("CVD_WALK", walk)
        for n_h1 in (nseq, 1000):
            _check(pt, n_h1, {"CVD_WALK": walk, "queue": cap}, r=r, want=want)
    monkeypatch.setenv("CVD_K1S_PERSIST", "0")
    assert pt.model.info()["persist_seqs"] == 0
    _check(pt, nseq, "block launch of the tiled buffer", r=r, want=want)


def test_nibble_packed_kernel_walking(pkg, pts, monkeypatch):
    """CVD_BITSLICE=0 at upload: the nibble-packed specialised kernel, in walk mode; with
    n_h1 = nseq every foreign window is a walking lane that leaves its rows and rebuilds its
    vector from the row key."""
    pt = pts["133_171_p0.01"]
    monkeypatch.setenv("CVD_BITSLICE", "0")
    monkeypatch.setenv("CVD_WALK", "1")
    monkeypatch.setenv("CVD_CHUNK", "0")
    model = pkg.Model(pt.det.dec, pt.p, LEARN, 200, 1.0, SEED).upload(0)
    inf = model.info()
    print("kernel", pkg.KERNEL_NAMES[inf["explicit_kernel"]], "lds_filter", inf["lds_filter"], "walk", inf["walk"])
    assert inf["explicit_kernel"] == 4 and inf["walk"] == 1, inf
    for n_h1 in (NSEQ, 64):
        _check(pt, n_h1, "nibble-packed, walking", model)


def test_chunked_launch_counts(pkg, pts, monkeypatch):
    """A chunked launch returns no sums: the counts.  The random and late-phase kinds are
    the chunks least likely to join (the rerun figures are printed)."""
    pt = pts["133_171_p0.05"]
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "192")
    for n_h1 in (NSEQ, 64):
        c = pt.det.detect(pt.model, pt.r, N, NSEQ, n_h1)
        torch.cuda.synchronize()
        st = pkg._lib.chunk_last()
        print("n_h1", n_h1, "chunk_last", st)
        assert st["C"] >= 2, st
        assert c.cpu().tolist() == counts_of(pt.want, n_h1), st
        assert pt.model.device_error() == 0


def test_detect_multi_three_models_one_buffer(pkg, pts, monkeypatch):
    """The three (133,171) models over the p = 0.05 buffer in one call: each model's sums
    equal its own reference on those words, so the p = 0.01 and p = 0.2 models score words of
    another p.  Models share a launch only where they share the specialised kernel's variant
    (multi_groups): the LDS-filter model of p = 0.01 runs alone, the p = 0.05 and p = 0.2
    models in one k1s_multi launch -- asserted, so that the shared launch is what runs."""
    three = [pts[i] for i in IDS[:3]]
    src = pts["133_171_p0.05"]
    groups = src.det.multi_groups([pt.model for pt in three], [NSEQ] * 3)
    print("multi_groups", groups)
    assert groups == [[0], [1, 2]], groups
    monkeypatch.setenv("CVD_CHUNK", "0")
    for walk in "01":
        monkeypatch.setenv("CVD_WALK", walk)
        for n_h1 in (NSEQ, 64):
            cnts = [torch.zeros(2, dtype=torch.int64, device=src.det.device) for _ in three]
            sums = [torch.full((NSEQ, 2), float("nan"), dtype=torch.float64, device=src.det.device) for _ in three]
            src.det.detect_multi([pt.model for pt in three], [src.r] * 3, N, [NSEQ] * 3, [n_h1] * 3, cnts, sums=sums)
            torch.cuda.synchronize()
            for pt, c, s in zip(three, cnts, sums):
                want = pt.want if pt is src else pt.om.score_words(src.words)[0]
                got = s.cpu().numpy()
                assert np.array_equal(got, want), (pt.mid, walk, n_h1, _mismatch(got, want))
                assert c.cpu().tolist() == counts_of(want, n_h1), (pt.mid, walk, n_h1)
                assert pt.model.device_error() == 0


@pytest.mark.parametrize("mid", IDS)
def test_scan_equals_score_words(pkg, pts, mid):
    """The 156 windows end to end as a byte-per-bit capture behind 13 junk bits, under the
    default environment (what a user's scan runs).  (171,133): two phases, the second the
    same windows read one bit later -- test_scan_phases' m = 6 counterpart, against the
    oracle instead of against detect."""
    pt = pts[mid]
    rng = np.random.default_rng(11)
    bits = np.concatenate([rng.integers(0, 2, JUNK).astype(np.uint8), F.serial_bits(pt.words).reshape(-1),
                           rng.integers(0, 2, 3).astype(np.uint8)])
    n_phase = 2 if pt.dec == (0o171, 0o133) else 1
    res = pt.det.scan(pt.model, bits, N, start=JUNK, n_phase=n_phase)
    assert res["logp1"].shape == res["logref"].shape == (NSEQ, n_phase)
    got = np.stack([res["logp1"][:, 0], res["logref"][:, 0]], axis=1)
    assert np.array_equal(got, pt.want), (mid, _mismatch(got, pt.want))
    assert np.array_equal(res["h1"][:, 0], pt.want[:, 0] > pt.want[:, 1])
    if n_phase == 2:
        late = np.stack([F.words_of_bits(bits[JUNK + 1 + 2 * N * i:JUNK + 1 + 2 * N * (i + 1)]) for i in range(NSEQ)])
        want1, _ = pt.om.score_words(late)
        got1 = np.stack([res["logp1"][:, 1], res["logref"][:, 1]], axis=1)
        assert np.array_equal(got1, want1), (mid, _mismatch(got1, want1))
        assert np.array_equal(res["offset"][:, 1], JUNK + 1 + 2 * N * np.arange(NSEQ))

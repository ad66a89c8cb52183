"""The bit-sliced m = 6 detector's one record load per step (cvd_k1s.h BsCursor::mid: a
filter-positive candidate's slot record, a known row's dense record -- which lies behind the
directory in the same device allocation -- or, for a lane that needs neither, a shared line)
against oracle.c_oracle's score_words: per-sequence sums (log P̂1, log T_ref) bit for bit, for
the decoder (133,171) with H2 streams of (171,133).

One model per kernel variant of the six-p sweep (learn_burn 200, laplace 1, seed 12345):
  ldsf  p = 0.01, learn_len 300,000: the LDS-filter kernel
  pf    p = 0.1,  learn_len 300,000: the pre-filter kernel (more rows than the LDS filter holds)
  mix   p = 0.05, the default learn_len: the pre-filter kernel, H1 and H2 waves alternating
260 sequences, 130 H1 then 130 H2: waves 0 and 1 hold H1 lanes only, wave 2 two H1 and 62 H2
lanes, wave 3 H2 lanes only, wave 4 four lanes.  N in {1, 5, 6, 7, 191, 192, 193, 773}: the
tail steps 1 to 5 of the six-step loop, the 192-step chunk grain, and enough steps for lanes
to leave their rows and come back.  A stream of N steps is the first N of the 773.

That the merged load is worked is asserted on the oracle's statistics before anything runs on
the GPU (test_inputs_work_the_merged_load): at p = 0.05, N = 773 every H1 stream re-enters
its rows at least once and spends a share of its steps strictly between 0.2 and 0.95 on a
row, so every H1 wave holds lanes on a row beside candidate lanes.  Measured on the oracle
(H1 streams, N = 773; rows learned): p = 0.05 share 0.521 to 0.885 (mean 0.720), 14 to 49
re-entries, 315,953 rows; p = 0.01 share 0.860 to 0.970, 1 to 24 re-entries, 14,007 rows;
p = 0.1 share 0.057 to 0.326, 6 to 43 re-entries, 263,589 rows.  H2 streams: share <= 0.04.
"""
import concurrent.futures

import numpy as np
import pytest
import torch

import foreign_streams as F
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

SEED = 12345
DEC = (0o133, 0o171)
NMAX, N_H1, NSEQ = 773, 130, 260
NS = [1, 5, 6, 7, 191, 192, 193, 773]
LDSF_ROWS = 98_304           # rows the LDS filter holds (cvd_host.cpp ldsf_max_rows, bit-sliced)
VARIANTS = {"ldsf": (0.01, 300_000), "pf": (0.1, 300_000), "mix": (0.05, None)}
VIDS = list(VARIANTS)
TILE = 9                     # 9 * 260 = 2,340 sequences: more than two blocks of 1,024 threads hold


def make_words(p):
    """[260, 773] received words: sequences 0..129 of (133,171), 130..259 of (171,133)."""
    tag = C.lib().oc_grid_tag(NMAX, p)
    g1, g2 = F.code(DEC), F.code(DEC[::-1])
    return np.stack([C.stream(g1 if q < N_H1 else g2, NMAX, p, SEED, tag, q) for q in range(NSEQ)]).astype(np.int32)


class Point:
    """One variant's oracle model, words, and per N the reference sums and stats (read-only)."""

    def __init__(self, vid, learn_len=None):
        self.vid = vid
        self.p, ll = VARIANTS[vid]
        self.learn_len = ll if learn_len is None else learn_len
        self.om = C.Model(F.code(DEC), self.p, self.learn_len, 200, 1.0, SEED)
        self.words = make_words(self.p)
        self.want, self.stats = {}, {}
        for n in NS:
            self.want[n], self.stats[n] = self.om.score_words(self.words[:, :n])
            self.want[n].setflags(write=False)
        self.words.setflags(write=False)

    def upload(self, pkg):
        self.det = pkg.Detector(1, 2, 6, F.gens(DEC), device=0)
        self.model = self.det.model(self.p, self.learn_len, 200, 1.0, SEED)
        self.r = {n: torch.from_numpy(F.pack_layout(self.words[:, :n]).view(np.int32)).cuda() for n in NS}


def counts_of(want, n_h1):
    lp, lr = want.T
    return [int((lp > lr)[:n_h1].sum()), int((lp <= lr)[n_h1:].sum())]


@pytest.fixture(scope="module")
def refs():
    with concurrent.futures.ThreadPoolExecutor(3) as ex:
        out = dict(zip(VIDS, ex.map(Point, VIDS)))
    if out["pf"].om.S <= LDSF_ROWS:   # (then the LDS-filter kernel would run it)
        out["pf"] = Point("pf", 1_000_000)
    return out


@pytest.fixture(scope="module")
def pts(pkg, refs):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    for pt in refs.values():
        pt.upload(pkg)
    return refs


def test_inputs_work_the_merged_load(refs):
    st = refs["mix"].stats[NMAX][:N_H1]
    share = st[:, 0] / NMAX
    print("p = 0.05, N = 773, H1 streams: on-row share min/mean/max %.3f %.3f %.3f, re-entries min/max %d %d"
          % (share.min(), share.mean(), share.max(), st[:, 1].min(), st[:, 1].max()))
    assert (st[:, 1] >= 1).all()
    assert (share > 0.2).all() and (share < 0.95).all()


def test_models_run_the_three_variants(pkg, pts):
    for vid, pt in pts.items():
        inf = pt.model.info()
        print(vid, "kernel", pkg.KERNEL_NAMES[inf["explicit_kernel"]], "lds_filter", inf["lds_filter"], "rows",
              inf["n_rows"], "learn_len_eff", inf["learn_len_eff"], "walk", inf["walk"])
        assert inf["explicit_kernel"] == 5, (vid, inf)           # the bit-sliced form
        assert inf["n_rows"] == pt.om.S, (vid, inf)
        assert inf["walk"] == 0, (vid, inf)                      # the lockstep loop by default
    ldsf, pf, mix = (pts[v].model.info() for v in VIDS)
    assert ldsf["lds_filter"] == 1 and ldsf["n_rows"] <= LDSF_ROWS, ldsf
    # (a bit-sliced model without the LDS filter runs the pre-filter kernel: cvd_host.cpp bs_pf_preferred)
    assert pf["lds_filter"] == 0 and pf["n_rows"] > LDSF_ROWS, pf
    assert not (2 * pf["n_rows"] < pf["learn_len_eff"]), pf      # no mixing (cvd_kernels.hip exp_args)
    assert mix["lds_filter"] == 0 and mix["kind"] == 1 and 2 * mix["n_rows"] < mix["learn_len_eff"], mix


def _sums(pt, model, r, n, nseq, n_h1, early=False):
    s = torch.full((nseq, 2), float("nan"), dtype=torch.float64, device=pt.det.device)
    c = pt.det.detect(model, r, n, nseq, n_h1, sums=None if early else s, early_decision=early)
    torch.cuda.synchronize()
    assert model.device_error() == 0
    return s.cpu().numpy(), c.cpu().tolist()


def _bad(got, want):
    return "sequences %s" % np.nonzero((got != want).any(axis=1))[0].tolist()[:20]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("vid", VIDS)
def test_block_and_persistent_launch(pts, monkeypatch, vid, n):
    pt = pts[vid]
    monkeypatch.setenv("CVD_CHUNK", "0")
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_K1S_PERSIST", "0")
    got, cnt = _sums(pt, pt.model, pt.r[n], n, NSEQ, N_H1)
    assert np.array_equal(got, pt.want[n]), (vid, n, "block", _bad(got, pt.want[n]))
    assert cnt == counts_of(pt.want[n], N_H1)
    # the work-queue launch: capped at two blocks, the 260 sequences nine times over
    monkeypatch.setenv("CVD_K1S_PERSIST", "1")
    monkeypatch.setenv("CVD_K1S_PERSIST_BLOCKS", "2")
    r, want = pt.r[n].repeat(1, TILE, 1).contiguous(), np.tile(pt.want[n], (TILE, 1))
    nseq = TILE * NSEQ
    cap = pt.model.info()["persist_seqs"]
    assert 0 < cap < nseq, cap
    got, cnt = _sums(pt, pt.model, r, n, nseq, nseq // 2)
    assert np.array_equal(got, want), (vid, n, "persistent", _bad(got, want))
    assert cnt == counts_of(want, nseq // 2)


@pytest.mark.parametrize("n", [7, 773])
def test_detect_multi_three_models(pts, monkeypatch, n):
    three = [pts[v] for v in VIDS]
    monkeypatch.setenv("CVD_CHUNK", "0")
    monkeypatch.setenv("CVD_WALK", "0")
    det = three[0].det
    cnts = [torch.zeros(2, dtype=torch.int64, device=det.device) for _ in three]
    sums = [torch.full((NSEQ, 2), float("nan"), dtype=torch.float64, device=det.device) for _ in three]
    det.detect_multi([pt.model for pt in three], [pt.r[n] for pt in three], n, [NSEQ] * 3, [N_H1] * 3, cnts, sums=sums)
    torch.cuda.synchronize()
    for pt, c, s in zip(three, cnts, sums):
        got = s.cpu().numpy()
        assert np.array_equal(got, pt.want[n]), (pt.vid, n, _bad(got, pt.want[n]))
        assert c.cpu().tolist() == counts_of(pt.want[n], N_H1), pt.vid
        assert pt.model.device_error() == 0


@pytest.mark.parametrize("vid", VIDS)
def test_chunked_launch_counts(pkg, pts, monkeypatch, vid):
    pt = pts[vid]
    monkeypatch.setenv("CVD_WALK", "0")
    monkeypatch.setenv("CVD_CHUNK", "1")
    monkeypatch.setenv("CVD_CHUNK_WARM", "192")
    c = pt.det.detect(pt.model, pt.r[NMAX], NMAX, NSEQ, N_H1)
    torch.cuda.synchronize()
    st = pkg._lib.chunk_last()
    print(vid, "chunk_last", st)
    assert st["C"] >= 2, st
    assert c.cpu().tolist() == counts_of(pt.want[NMAX], N_H1), st
    assert pt.model.device_error() == 0


@pytest.mark.parametrize("vid", VIDS)
def test_early_decision_counts(pts, monkeypatch, vid):
    pt = pts[vid]
    monkeypatch.setenv("CVD_CHUNK", "0")
    monkeypatch.setenv("CVD_WALK", "0")
    for n in (193, NMAX):
        _, cnt = _sums(pt, pt.model, pt.r[n], n, NSEQ, N_H1, early=True)
        assert cnt == counts_of(pt.want[n], N_H1), (vid, n)


@pytest.mark.parametrize("vid", VIDS)
def test_forced_walk(pts, monkeypatch, vid):
    """CVD_WALK=1: the walking code object, whose ACS steps take the candidate-only record
    load so that a lane which has just left its rows keeps the record its walk loaded."""
    pt = pts[vid]
    monkeypatch.setenv("CVD_CHUNK", "0")
    monkeypatch.setenv("CVD_WALK", "1")
    monkeypatch.setenv("CVD_K1S_PERSIST", "0")
    assert pt.model.info()["walk"] == 1
    for n in NS:
        got, cnt = _sums(pt, pt.model, pt.r[n], n, NSEQ, N_H1)
        assert np.array_equal(got, pt.want[n]), (vid, n, _bad(got, pt.want[n]))
        assert cnt == counts_of(pt.want[n], N_H1)

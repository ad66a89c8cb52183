"""decode_frames_soft_punctured, decode_frames_tailbiting_soft_punctured and
decode_frames_llr_punctured on the GPU, exact equality throughout.  The contract is one rule: the
result is the unpunctured soft call's on the frames depunctured one by one.  So every case is
compared (a) with numpy oracles on the frames that psoft_cases depunctures from the header's text
-- llr_cases.viterbi_frame and a re-encoding for the terminated call, llr_cases.reference_batch for
the soft-output call -- and (b) in every field with the unpunctured sibling on that host-depunctured
capture, which is the tail-biting call's oracle (decode_frames_tailbiting_soft is pinned by its own
tests).  Shapes: S below, at and above a wave and four states per lane; n = 2 and 3; periods that
do and do not divide 64; frame lengths around the pattern's period, the soft-output segment (32),
the wave chunk (64) and the staging segment (1024); offsets at every alignment class that the
16-byte staging distinguishes."""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import llr_cases as LC
import psoft_cases as PC
from conftest import ROOT

pytestmark = pytest.mark.gpu

BOUNDARIES = [(0, 0), (None, None), (5, None), (None, 6), (5, 6)]
TOTALS = ("T", "F", "words", "decoded", "skipped", "total_distance")
KEYS = {
    "frames": TOTALS + ("total_errors", "total_counted", "ber"),
    "tail": TOTALS + ("total_errors", "total_counted", "ber", "fallback", "open", "total_laps"),
    "llr": TOTALS + ("total_zeros", "total_saturated"),
}


def same(kind, got, want):
    """Every tensor and every total of two result dicts."""
    assert set(got) == set(want)
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
            assert torch.equal(got[k], v), (kind, k, (got[k] != v).nonzero()[:5].tolist())
    for k in KEYS[kind]:
        assert got[k] == want[k], (kind, k, got[k], want[k])


def offsets_for(span, F, rng):
    """F offsets of frames of `span` values that do not overlap, their residues mod 16 running through
    0, 1, 15 and random ones; the capture ends with the last frame's last value."""
    off, o = [], 16
    for f in range(F):
        r = (0, 1, 15)[f] if f < 3 else int(rng.integers(0, 16))
        o = (o + 15) // 16 * 16 + r
        off.append(o)
        o += span + int(rng.integers(0, 9))
    return np.array(off, dtype=np.int64), off[-1] + span


@functools.lru_cache(maxsize=None)
def capture(m, n, pat, T, F, s0, e, kind, seed=0):
    """A capture of F punctured soft frames (computed once, not written to): the values, the
    offsets, the pattern, the host-depunctured capture and the frames' offsets in it."""
    pn, keep = PC.PATTERNS[pat]
    assert pn == n
    gen = LC.gen_of(m, n)
    rng = np.random.default_rng(seed + 7919 * m + 31 * n + 101 * T + len(pat) + sum(keep))
    offsets, nvals = offsets_for(PC.pos(T, keep), F, rng)
    frames = [PC.punctured_frame(rng, gen, n, m, keep, T, s0, e, kind) for _ in range(F)]
    cap = PC.place(frames, offsets, nvals, rng)
    dep, dep_off = PC.depunctured_capture(cap, keep, n, T, offsets)
    for a in (cap, dep):
        a.setflags(write=False)
    return cap, offsets, keep, dep, dep_off


def check_frames(pkg, m, n, keep, T, cap, offsets, dep, dep_off, s0, e, place=None):
    """The terminated call against the numpy oracle and against decode_frames_soft on dep."""
    gen = LC.gen_of(m, n)
    place = dict(offsets=offsets) if place is None else place
    res = pkg.decode_frames_soft_punctured(n, m, gen, keep, cap, T, start_state=s0, end_state=e, **place)

    left = [4]

    def independent(v, dist, u, sT):
        if (T << m) <= 30000 and left[0] > 0:                 # the plain-Python decoder, where it is quick
            left[0] -= 1
            d2, u2, sT2 = LC.viterbi_frame(gen, n, m, v, T, s0, e)
            assert (dist, sT) == (d2, sT2) and np.array_equal(u, u2)

    bits, frames, stats = PC.reference_frames(gen, n, m, cap, keep, T, offsets, s0, e, independent)
    got = res["frames"].cpu().numpy()
    assert np.array_equal(got, frames), (np.argwhere(got != frames)[:5], got[:3], frames[:3])
    assert np.array_equal(res["bits"].cpu().numpy(), bits)
    assert [res["total_distance"], res["decoded"], res["skipped"], res["total_errors"], res["total_counted"],
            res["words"]] == stats
    same("frames", res, pkg.decode_frames_soft(n, m, gen, dep, T, offsets=dep_off, start_state=s0, end_state=e))
    return res


def check_llr(pkg, m, n, keep, T, cap, offsets, dep, dep_off, s0, e, place=None):
    """The soft-output call against llr_cases.reference_batch and against decode_frames_llr on dep."""
    gen = LC.gen_of(m, n)
    place = dict(offsets=offsets) if place is None else place
    res = pkg.decode_frames_llr_punctured(n, m, gen, keep, cap, T, start_state=s0, end_state=e, **place)
    llr, bits, frames, stats = LC.reference_batch(gen, n, m, dep, T, dep_off, s0, e)
    assert np.array_equal(res["llr"].cpu().numpy(), llr), np.argwhere(res["llr"].cpu().numpy() != llr)[:5]
    assert np.array_equal(res["bits"].cpu().numpy(), bits)
    assert np.array_equal(res["frames"].cpu().numpy(), frames), (res["frames"].cpu().numpy()[:3], frames[:3])
    assert [res["total_distance"], res["decoded"], res["skipped"], res["total_zeros"], res["total_saturated"],
            res["words"]] == stats
    same("llr", res, pkg.decode_frames_llr(n, m, gen, dep, T, offsets=dep_off, start_state=s0, end_state=e))
    return res


def check_both(pkg, m, n, pat, T, F, s0, e, kind="noisy"):
    cap, offsets, keep, dep, dep_off = capture(m, n, pat, T, F, s0, e, kind)
    return (check_frames(pkg, m, n, keep, T, cap, offsets, dep, dep_off, s0, e),
            check_llr(pkg, m, n, keep, T, cap, offsets, dep, dep_off, s0, e))


# ── terminated frames and soft output ──

N2 = ["all2", "dvb:2/3", "dvb:3/4", "dvb:7/8", "p16"]
SHAPES = [(m, 2, p) for m in (3, 6, 7, 8) for p in N2] + [(m, 3, p) for m in (6, 8) for p in ("all3", "n3")]


@pytest.mark.parametrize("m,n,pat", SHAPES)
def test_codes_and_patterns(pkg, m, n, pat):
    """Every code shape against every pattern at T = 97: two wave chunks and four soft-output
    segments with ragged ends; terminated frames and free ones."""
    check_both(pkg, m, n, pat, 97, 5, 0, 0)
    check_both(pkg, m, n, pat, 97, 3, None, None)


@pytest.mark.parametrize("m,n,pat", [(6, 2, "all2"), (8, 3, "all3")])
def test_all_kept_is_the_unpunctured_call(pkg, m, n, pat):
    """Period 1 with every output kept: the same capture through the unpunctured calls."""
    cap, offsets, keep, _, _ = capture(m, n, pat, 97, 5, 0, 0, "noisy")
    gen = LC.gen_of(m, n)
    same("frames", pkg.decode_frames_soft_punctured(n, m, gen, keep, cap, 97, offsets=offsets),
         pkg.decode_frames_soft(n, m, gen, cap, 97, offsets=offsets))
    same("llr", pkg.decode_frames_llr_punctured(n, m, gen, keep, cap, 97, offsets=offsets),
         pkg.decode_frames_llr(n, m, gen, cap, 97, offsets=offsets))
    same("tail", pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, cap, 97, offsets=offsets),
         pkg.decode_frames_tailbiting_soft(n, m, gen, cap, 97, offsets=offsets))


LENGTHS = [1, 31, 32, 33, 63, 64, 65, 97, 1023, 1024, 1025]


@pytest.mark.parametrize("m,n,pat", [(6, 2, "dvb:3/4"), (3, 2, "dvb:7/8"), (7, 2, "p16"), (8, 3, "n3"), (6, 2, "dvb:2/3")])
@pytest.mark.parametrize("T", LENGTHS + ["period-1", "period", "period+1"])
def test_frame_lengths(pkg, m, n, pat, T):
    """Around the period, the soft-output segment, the wave chunk and the staging segment."""
    period = len(PC.PATTERNS[pat][1])
    if isinstance(T, str):
        T = period + {"period-1": -1, "period": 0, "period+1": 1}[T]
        if T < 1 or T in LENGTHS:
            T = period + 16                                   # (nothing new at this pattern: a length of its own)
    e = 0 if T >= m else None                                 # both states fixed need T >= m
    check_both(pkg, m, n, pat, T, 3 if T > 1000 else 6, 0, e)


@pytest.mark.parametrize("s0,e", BOUNDARIES)
@pytest.mark.parametrize("m,n,pat", [(6, 2, "dvb:3/4"), (8, 3, "n3")])
def test_boundary_states(pkg, m, n, pat, s0, e):
    check_both(pkg, m, n, pat, 70, 5, s0, e)


@pytest.mark.parametrize("kind", ["noisy", "m128", "zero", "pm1"])
@pytest.mark.parametrize("m,n,pat", [(6, 2, "dvb:3/4"), (7, 2, "dvb:7/8"), (6, 3, "n3")])
def test_inputs(pkg, m, n, pat, kind):
    """-128 and 0 among the kept values, an all-zero frame, +-1 values with their many ties."""
    T, F = 70, 5
    cap, offsets, keep, dep, dep_off = capture(m, n, pat, T, F, 0, None, kind)
    span = PC.pos(T, keep)
    kept = np.concatenate([cap[o:o + span] for o in offsets])
    if kind == "m128":
        assert (kept == -128).any()
    if kind == "pm1":
        assert set(np.unique(kept)) <= {-1, 0, 1}
    assert (kept == 0).any()                                  # erasures among the kept values
    res, rl = check_both(pkg, m, n, pat, T, F, 0, None, kind)
    counted = res["counted"].cpu().numpy()
    assert np.array_equal(counted, [(cap[o:o + span] != 0).sum() for o in offsets])      # zeros are not counted
    assert res["total_counted"] == int((kept != 0).sum()) < F * span
    if kind == "zero":
        assert res["total_counted"] == 0 and res["total_distance"] == 0 and not res["bits"].any()
        assert rl["total_zeros"] == F * T


def test_strides(pkg):
    """Stride mode with gaps between the frames, from a start that is not aligned; the last frame
    ends with the capture."""
    m, n, pat, T, F, start = 6, 2, "dvb:3/4", 70, 7, 5
    keep = PC.PATTERNS[pat][1]
    gen, rng = LC.gen_of(m, n), np.random.default_rng(11)
    span = PC.pos(T, keep)
    stride = span + 13
    offsets = start + stride * np.arange(F, dtype=np.int64)
    frames = [PC.punctured_frame(rng, gen, n, m, keep, T, 0, 0, "noisy") for _ in range(F)]
    cap = PC.place(frames, offsets, int(offsets[-1]) + span, rng)
    dep, dep_off = PC.depunctured_capture(cap, keep, n, T, offsets)
    place = dict(F=F, start=start, stride=stride)
    check_frames(pkg, m, n, keep, T, cap, offsets, dep, dep_off, 0, 0, place)
    check_llr(pkg, m, n, keep, T, cap, offsets, dep, dep_off, 0, 0, place)
    same("tail", pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, cap, T, **place),
         pkg.decode_frames_tailbiting_soft(n, m, gen, dep, T, offsets=dep_off))
    # the default stride is the punctured span: the frames follow one another
    res = pkg.decode_frames_soft_punctured(n, m, gen, keep, cap[:5 * span], T)
    assert res["F"] == 5 and res["decoded"] == 5
    with pytest.raises(ValueError):
        pkg.decode_frames_soft_punctured(n, m, gen, keep, cap, T, F=F, start=start + 1, stride=stride)


def test_offsets(pkg):
    """Offset mode: negative, repeated and overlapping offsets; o + span = nvals is decoded,
    o + span = nvals + 1 is skipped (with n T in the place of the span both would be skipped)."""
    m, n, pat, T = 6, 2, "dvb:3/4", 70
    keep = PC.PATTERNS[pat][1]
    gen, rng = LC.gen_of(m, n), np.random.default_rng(12)
    span = PC.pos(T, keep)
    assert span == 94
    nvals = 500
    good = np.array([16, 129, 255, 300], dtype=np.int64)        # 255 + 94 > 300: the last two overlap
    frames = [PC.punctured_frame(rng, gen, n, m, keep, T, 0, None, "noisy") for _ in good]
    cap = PC.place(frames, good, nvals, rng)
    offsets = np.array([16, -1, 129, 129, -span, 255, 300, nvals - span, nvals - span + 1, nvals, 1 << 40, 16],
                       dtype=np.int64)
    dep, dep_off = PC.depunctured_capture(cap, keep, n, T, offsets)
    assert (dep_off < 0).tolist() == [False, True, False, False, True, False, False, False, True, True, True, False]
    res = check_frames(pkg, m, n, keep, T, cap, offsets, dep, dep_off, 0, None)
    assert res["skipped"] == 5 and res["status"].cpu().tolist() == [0, 1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 0]
    assert not res["bits"][res["status"] == 1].any()
    check_llr(pkg, m, n, keep, T, cap, offsets, dep, dep_off, 0, None)
    same("tail", pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, cap, T, offsets=offsets),
         pkg.decode_frames_tailbiting_soft(n, m, gen, dep, T, offsets=dep_off))


def test_same_result_on_every_launch(pkg, monkeypatch):
    """Two batches of the terminated call, fewer waves than frames in the other two."""
    m, n, pat, T, F = 6, 2, "dvb:7/8", 33, 150
    cap, offsets, keep, dep, dep_off = capture(m, n, pat, T, F, 0, 0, "noisy")
    gen = LC.gen_of(m, n)
    calls = {"frames": lambda: pkg.decode_frames_soft_punctured(n, m, gen, keep, cap, T, offsets=offsets),
             "llr": lambda: pkg.decode_frames_llr_punctured(n, m, gen, keep, cap, T, offsets=offsets),
             "tail": lambda: pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, cap, T, offsets=offsets)}
    for var in ("CVD_FRAMES_BATCH_BYTES", "CVD_LLR_WAVES", "CVD_TAILBITE_WAVES"):
        monkeypatch.delenv(var, raising=False)
    want = {k: f() for k, f in calls.items()}
    check_frames(pkg, m, n, keep, T, cap, offsets, dep, dep_off, 0, 0)
    monkeypatch.setenv("CVD_FRAMES_BATCH_BYTES", "4096")      # a batch is never below 64 frames: 64 + 64 + 22
    monkeypatch.setenv("CVD_LLR_WAVES", "7")
    monkeypatch.setenv("CVD_TAILBITE_WAVES", "7")
    assert pkg.lib().cvd_viterbi_frames_workspace_bytes(n, m, T, F, 1) == 64 * 64 * 8
    for k, f in calls.items():
        same(k, f(), want[k])


def test_no_frames(pkg):
    gen, cap = LC.gen_of(6, 2), np.zeros(64, dtype=np.int8)
    for fn in (pkg.decode_frames_soft_punctured, pkg.decode_frames_tailbiting_soft_punctured,
               pkg.decode_frames_llr_punctured):
        res = fn(2, 6, gen, "dvb:3/4", cap, 100)                # 134 values do not fit: no frames
        assert res["F"] == 0 and res["decoded"] == 0 and tuple(res["bits"].shape) == (0, 16)


# ── tail-biting frames ──

TAIL = [(6, 2, "dvb:3/4", 40), (6, 2, "dvb:3/4", 64), (6, 2, "dvb:3/4", 100), (6, 2, "dvb:2/3", 40), (3, 2, "dvb:7/8", 64),
        (7, 2, "p16", 100), (8, 3, "n3", 40), (6, 3, "n3", 100), (8, 2, "dvb:7/8", 64)]
SIGMAS = (0.3, 0.5, 0.7, 0.9, 0.3, 1.1, 0.5, 1.3)              # of the amplitude; per frame, quiet to hopeless


@functools.lru_cache(maxsize=None)
def tail_case(pkg, m, n, pat, T):
    """Eight tail-biting frames, and the reference: decode_frames_tailbiting_soft on the
    host-depunctured capture."""
    keep = PC.PATTERNS[pat][1]
    gen = LC.gen_of(m, n)
    rng = np.random.default_rng(4242 + 7919 * m + 31 * n + T + sum(keep))
    offsets, nvals = offsets_for(PC.pos(T, keep), len(SIGMAS), rng)
    frames = [PC.tailbiting_frame(rng, gen, n, m, keep, T, s) for s in SIGMAS]
    cap = PC.place(frames, offsets, nvals, rng)
    dep, dep_off = PC.depunctured_capture(cap, keep, n, T, offsets)
    ref = pkg.decode_frames_tailbiting_soft(n, m, gen, dep, T, offsets=dep_off)
    return cap, offsets, keep, dep, dep_off, ref


def test_tailbiting_reference_is_informative(pkg):
    """The inputs exercise the laps: over the cases the reference needs more than one lap for some
    frames and closes (status 0) most of them."""
    laps = np.concatenate([tail_case(pkg, *c)[5]["laps"].cpu().numpy() for c in TAIL])
    status = np.concatenate([tail_case(pkg, *c)[5]["status"].cpu().numpy() for c in TAIL])
    print("laps", np.bincount(laps).tolist(), "status", np.bincount(status).tolist())
    assert (laps > 1).sum() >= 3
    assert (status == 0).sum() > len(status) // 2


@pytest.mark.parametrize("m,n,pat,T", TAIL)
def test_tailbiting(pkg, m, n, pat, T):
    cap, offsets, keep, dep, dep_off, ref = tail_case(pkg, m, n, pat, T)
    gen = LC.gen_of(m, n)
    res = pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, cap, T, offsets=offsets)
    same("tail", res, ref)
    assert tuple(res["frames"].shape) == (len(SIGMAS), 8)
    span = PC.pos(T, keep)
    assert res["counted"].cpu().tolist() == [int((cap[o:o + span] != 0).sum()) for o in offsets]
    for laps in (1, 2):
        same("tail", pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, cap, T, offsets=offsets, max_laps=laps),
             pkg.decode_frames_tailbiting_soft(n, m, gen, dep, T, offsets=dep_off, max_laps=laps))


def test_tailbiting_decision_words_in_memory(pkg, monkeypatch):
    """Frames whose decision words do not fit the LDS limit take the workspace placement."""
    m, n, pat, T = 6, 2, "dvb:3/4", 100
    cap, offsets, keep, dep, dep_off, ref = tail_case(pkg, m, n, pat, T)
    monkeypatch.setenv("CVD_TAILBITE_LDS_BYTES", "512")
    assert pkg.lib().cvd_viterbi_tailbiting_workspace_bytes(n, m, T, 8, 1) > 0
    same("tail", pkg.decode_frames_tailbiting_soft_punctured(n, m, LC.gen_of(m, n), keep, cap, T, offsets=offsets), ref)


# ── the command line ──

def test_decode_cli(pkg, tmp_path):
    """decode --frame T --format soft --puncture dvb:3/4 in a fresh process: decoded.npy and the
    CSV rows equal the Python call's."""
    m, n, T, F, start = 6, 2, 70, 6, 3
    keep = PC.PATTERNS["dvb:3/4"][1]
    gen, rng = LC.gen_of(m, n), np.random.default_rng(13)          # (6, 2): oct 133,171
    span = PC.pos(T, keep)
    stride = span + 6
    offsets = start + stride * np.arange(F, dtype=np.int64)
    cap = PC.place([PC.punctured_frame(rng, gen, n, m, keep, T, 0, 0, "noisy") for _ in range(F)], offsets,
                   int(offsets[-1]) + span, rng)
    npy, out = str(tmp_path / "cap.npy"), str(tmp_path / "res")
    np.save(npy, cap)
    pkg_name = os.path.basename(os.path.dirname(pkg.__file__))
    cmd = [sys.executable, "-m", pkg_name, "decode", "--code", "oct:133,171", "--input", npy, "--format", "soft",
           "--puncture", "dvb:3/4", "--start", str(start), "--frame", str(T), "--frame-stride", str(stride),
           "--save-dir", out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    want = pkg.decode_frames_soft_punctured(n, m, gen, "dvb:3/4", cap, T, start=start, stride=stride)
    assert want["F"] == F and want["decoded"] == F
    assert np.array_equal(np.load(os.path.join(out, "decoded.npy")), want["bits"].cpu().numpy())
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "offset", "status", "distance", "errors", "counted", "start_state", "end_state"]
    rec = want["frames"].cpu().numpy()
    assert [[int(x) for x in r] for r in rows[1:]] == \
        [[i, int(offsets[i]), rec[i, 3], rec[i, 0], rec[i, 4], rec[i, 5], rec[i, 1], rec[i, 2]] for i in range(F)]
    assert f"Decoded {F} frames of {T} steps (0 skipped)" in run.stdout

"""cvd_viterbi_decode_frames_llr on the GPU against the sequential decoder of llr_cases.py, which
is written from the text of include/cvd.h: exact equality of the values, the bits, all six fields
of every record and all six totals, at the smallest shapes at which the kernel can go wrong (S
below, at and above a wave; frames of one segment, of whole segments and with a ragged last one;
every boundary condition; erasures, -128, all-zero and +-1 inputs; every kind of placement; a
launch with fewer waves than frames), the consistency with decode_frames_soft that the header
states, and the decode subcommand's --llr."""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import llr_cases as LC
from conftest import ROOT

pytestmark = pytest.mark.gpu

CODES = [(m, 2) for m in range(1, 9)] + [(6, 3), (8, 3)]


@functools.lru_cache(maxsize=None)
def capture(m, n, T, F, s0, e, kind, gap=5, lead=3, seed=0):
    """A soft capture of F frames of T steps, `gap` values of noise between them and `lead` before
    the first, the frames' offsets, and the reference's outputs (computed once, not written to)."""
    gen = LC.gen_of(m, n)
    rng = np.random.default_rng(seed + 7919 * m + 31 * n + T)
    stride = n * T + gap
    soft = rng.integers(-20, 21, lead + F * stride, dtype=np.int8)
    offsets = lead + stride * np.arange(F, dtype=np.int64)
    for o in offsets:
        soft[o:o + n * T] = LC.soft_frame(rng, gen, n, m, T, s0, e, kind)[0]
    ref = LC.reference_batch(gen, n, m, soft, T, offsets, s0, e)
    for a in (soft, offsets) + ref[:3]:
        a.setflags(write=False)
    return soft, offsets, stride, ref


def padded_rows(res):
    """The F rows of 32 w values behind the [F, T] view."""
    w = res["words"]
    return res["llr"].as_strided((res["F"], 32 * w), (32 * w, 1)).cpu().numpy()


def assert_equals_reference(res, ref, T):
    llr, bits, frames, stats = ref
    F, w = llr.shape[0], (T + 31) // 32
    assert res["llr"].dtype == torch.int16 and tuple(res["llr"].shape) == (F, T)
    got = padded_rows(res)
    assert np.array_equal(got[:, :T], llr), np.argwhere(got[:, :T] != llr)[:5]
    assert not got[:, T:].any()                                  # values at or past T are 0
    assert np.array_equal(res["bits"].cpu().numpy(), bits)
    assert np.array_equal(res["frames"].cpu().numpy(), frames), (res["frames"].cpu().numpy(), frames)
    assert [res["total_distance"], res["decoded"], res["skipped"], res["total_zeros"], res["total_saturated"],
            res["words"]] == stats
    for name, col in (("distance", 0), ("zeros", 1), ("end_states", 2), ("status", 3), ("weakest", 4), ("saturated", 5)):
        assert np.array_equal(res[name].cpu().numpy(), frames[:, col]), name
    assert res["T"] == T and res["F"] == F and res["words"] == w


def run_case(pkg, m, n, T, F, s0, e, kind="noisy"):
    soft, offsets, stride, ref = capture(m, n, T, F, s0, e, kind)
    res = pkg.decode_frames_llr(n, m, LC.gen_of(m, n), soft, T, F=F, start=3, stride=stride, start_state=s0, end_state=e)
    assert_equals_reference(res, ref, T)
    return res, ref


@pytest.mark.parametrize("m,n", CODES)
def test_code_shapes(pkg, m, n):
    """Four segments with a ragged last one (two checkpoints), terminated frames and free ones."""
    run_case(pkg, m, n, 102, 5, 0, 0)
    run_case(pkg, m, n, 102, 3, None, None)


@pytest.mark.parametrize("T", [1, 6, 7, 31, 32, 33, 63, 64, 65, 96, 97, 100, 1025])
@pytest.mark.parametrize("m,n", [(3, 2), (6, 2), (7, 2), (8, 3)])
def test_frame_lengths(pkg, m, n, T):
    F = 2 if T > 1000 else 4
    run_case(pkg, m, n, T, F, 0, None)
    if T >= m:
        run_case(pkg, m, n, T, F, 0, 0)


@pytest.mark.parametrize("m", [1, 2, 8])
def test_frame_lengths_around_m(pkg, m):
    for T in (1, m, m + 1):
        run_case(pkg, m, 2, T, 4, None, 0)
        if T >= m:
            run_case(pkg, m, 2, T, 4, 0, 0)


@pytest.mark.parametrize("m,n", [(3, 2), (6, 2), (6, 3), (7, 2), (8, 2)])
def test_boundary_states(pkg, m, n):
    S = 1 << m
    s, e = S - 2, (S // 2) | 1
    for s0, e0 in ((0, 0), (None, None), (s, None), (None, e), (s, e)):
        res, ref = run_case(pkg, m, n, 45, 4, s0, e0)
        sat = (np.abs(ref[0]) == LC.SAT).sum(axis=1)
        assert (sat == (m if e0 is not None else 0)).all()       # the tail, and nothing else


@pytest.mark.parametrize("kind", ["m128", "zero", "pm1"])
@pytest.mark.parametrize("m,n", [(2, 2), (6, 2), (8, 2)])
def test_inputs(pkg, m, n, kind):
    T = 50
    for s0, e in ((0, 0), (None, None)):
        res, ref = run_case(pkg, m, n, T, 4, s0, e, kind)
        if kind == "zero":                                       # nothing is known: every unsaturated value is 0
            unsat = T - (m if e is not None else 0)
            assert (res["zeros"].cpu().numpy() == unsat).all() and res["total_distance"] == 0
            assert not (padded_rows(res)[:, :unsat]).any()
        if kind == "pm1":
            assert res["total_zeros"] > 0                        # many ties
    if kind == "m128":
        assert (capture(m, n, T, 4, 0, 0, kind)[0] == -128).any()


def test_hard_bits_through_soft_from_bits(pkg):
    m, n, T, F = 6, 2, 40, 3
    gen = LC.gen_of(m, n)
    rng = np.random.default_rng(11)
    bits = np.concatenate([LC.encode(gen, n, m, np.r_[rng.integers(0, 2, T - m), np.zeros(m, dtype=np.int64)], 0)[0]
                           for _ in range(F)])
    bits[rng.random(bits.size) < 0.04] ^= 1
    soft = pkg.soft_from_bits(bits, 3)
    res = pkg.decode_frames_llr(n, m, gen, soft, T)
    assert res["F"] == F
    assert_equals_reference(res, LC.reference_batch(gen, n, m, soft, T, n * T * np.arange(F), 0, 0), T)
    assert not (padded_rows(res)[:, :T - m] % 3).any()         # costs are multiples of the amplitude


def test_offsets(pkg):
    """Offset mode: negative offsets and offsets past the end are skipped (zero rows, the skip
    record), frames overlap and repeat, offsets are odd and unaligned."""
    m, n, T = 6, 2, 70
    gen = LC.gen_of(m, n)
    soft = capture(m, n, T, 5, 0, 0, "noisy")[0]
    N = len(soft)
    offsets = np.array([3, -1, 3 + n * T + 5, N - n * T + 1, 3, 10, 11, -(1 << 40), N - n * T, N, 1 << 40, 77],
                       dtype=np.int64)
    for s0, e in ((0, 0), (None, None)):
        ref = LC.reference_batch(gen, n, m, soft, T, offsets, s0, e)
        assert ref[3][1] == 7 and ref[3][2] == 5
        res = pkg.decode_frames_llr(n, m, gen, soft, T, offsets=offsets, start_state=s0, end_state=e)
        assert_equals_reference(res, ref, T)
        skipped = res["status"].cpu().numpy() == 1
        assert not padded_rows(res)[skipped].any() and not res["bits"].cpu().numpy()[skipped].any()
        assert (res["frames"].cpu().numpy()[skipped] == [0, 0, -1, 1, 0, 0]).all()
    # a device tensor of offsets, and only skipped frames
    res = pkg.decode_frames_llr(n, m, gen, soft, T, offsets=torch.tensor([-5, N], dtype=torch.int64, device="cuda"))
    assert_equals_reference(res, LC.reference_batch(gen, n, m, soft, T, [-5, N], 0, 0), T)


def test_strides(pkg):
    """Stride mode: a stride larger than the frame (capture() has a gap), an odd start, frames
    that follow one another, and overlapping frames at stride 1."""
    m, n, T = 5, 2, 37
    gen = LC.gen_of(m, n)
    soft, offsets, stride, ref = capture(m, n, T, 6, 0, None, "noisy")
    assert stride > n * T and offsets[0] % 2 == 1
    run_case(pkg, m, n, T, 6, 0, None)
    for start, st, F in ((0, n * T, 6), (1, 1, 9), (5, 3, None)):
        res = pkg.decode_frames_llr(n, m, gen, soft, T, F=F, start=start, stride=st, start_state=None, end_state=None)
        off = start + st * np.arange(res["F"])
        assert F is None or res["F"] == F
        assert_equals_reference(res, LC.reference_batch(gen, n, m, soft, T, off, None, None), T)


@pytest.mark.parametrize("m,n", [(4, 2), (6, 2), (8, 2)])
def test_same_result_on_every_launch(pkg, monkeypatch, m, n):
    """F = 10 frames on 3 waves: the grid stride, a wave's slice of checkpoints reused."""
    T, F = 100, 10
    soft, offsets, stride, ref = capture(m, n, T, F, 0, 0, "noisy")
    gen = LC.gen_of(m, n)
    monkeypatch.setenv("CVD_LLR_WAVES", "3")
    assert pkg.lib().cvd_viterbi_llr_workspace_bytes(n, m, T, F) == 3 * 2 * (4 << m)
    a = pkg.decode_frames_llr(n, m, gen, soft, T, F=F, start=3, stride=stride)
    assert_equals_reference(a, ref, T)
    monkeypatch.setenv("CVD_LLR_WAVES", "1")
    b = pkg.decode_frames_llr(n, m, gen, soft, T, F=F, start=3, stride=stride)
    assert_equals_reference(b, ref, T)
    monkeypatch.delenv("CVD_LLR_WAVES")
    assert_equals_reference(pkg.decode_frames_llr(n, m, gen, soft, T, F=F, start=3, stride=stride), ref, T)


@pytest.mark.parametrize("kind", ["noisy", "pm1"])
@pytest.mark.parametrize("m,n", [(2, 2), (6, 2), (6, 3), (7, 2), (8, 3)])
def test_consistent_with_decode_frames_soft(pkg, m, n, kind):
    """On the same arguments: the distance and the end state are decode_frames_soft's, and so is
    every bit whose value is not 0 -- a theorem, so no exception is allowed."""
    T, F = 90, 40
    gen = LC.gen_of(m, n)
    S = 1 << m
    for s0, e in ((0, 0), (None, None), (S - 1, None), (None, 1)):
        rng = np.random.default_rng(100 * m + n)
        soft = np.concatenate([LC.soft_frame(rng, gen, n, m, T, s0, e, kind, sigma=0.9)[0] for _ in range(F)])
        a = pkg.decode_frames_llr(n, m, gen, soft, T, start_state=s0, end_state=e)
        b = pkg.decode_frames_soft(n, m, gen, soft, T, start_state=s0, end_state=e)
        assert a["F"] == b["F"] == F
        assert torch.equal(a["distance"], b["distance"]) and torch.equal(a["end_states"], b["end_states"])
        assert a["total_distance"] == b["total_distance"]
        L = a["llr"].cpu().numpy()
        ua = np.unpackbits(a["bits"].cpu().numpy(), axis=1, bitorder="little")[:, :T]
        ub = np.unpackbits(b["bits"].cpu().numpy(), axis=1, bitorder="little")[:, :T]
        assert np.array_equal(ua, L > 0)
        assert np.array_equal(ua[L != 0], ub[L != 0])
        if kind == "pm1":
            assert (L == 0).any()


def test_argument_errors(pkg):
    gen = LC.gen_of(6, 2)
    soft = np.zeros(1000, dtype=np.int8)
    with pytest.raises(ValueError):
        pkg.decode_frames_llr(2, 6, gen, soft, 5)                 # both states fixed and T < m
    with pytest.raises(ValueError):
        pkg.decode_frames_llr(2, 6, gen, soft, 100, F=6)
    with pytest.raises(pkg.CvdError, match="viterbi_decode_frames_llr"):
        pkg.decode_frames_llr(2, 9, [[[1] * 10], [[1, 0, 1, 1, 1, 0, 0, 0, 1, 1]]], soft, 100)
    res = pkg.decode_frames_llr(2, 6, gen, soft, 100, F=0)
    assert res["F"] == 0 and tuple(res["llr"].shape) == (0, 100) and res["decoded"] == 0


def test_decode_cli_llr(pkg, tmp_path):
    """decode --frame T --format soft --llr in a fresh process: llr.npy, decoded.npy and the CSV
    rows equal the Python call's."""
    m, n, T, F = 6, 2, 70, 6
    soft, offsets, stride, ref = capture(m, n, T, F, 0, 0, "noisy")
    npy, out = str(tmp_path / "cap.npy"), str(tmp_path / "res")
    np.save(npy, soft)
    pkg_name = os.path.basename(os.path.dirname(pkg.__file__))
    cmd = [sys.executable, "-m", pkg_name, "decode", "--code", "oct:133,171", "--input", npy, "--format", "soft",
           "--start", "3", "--frame", str(T), "--frame-stride", str(stride), "--llr", "--save-dir", out]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    want = pkg.decode_frames_llr(n, m, LC.gen_of(m, n), soft, T, start=3, stride=stride)
    assert want["F"] == F
    got = np.load(os.path.join(out, "llr.npy"))
    assert got.dtype == np.int16 and got.shape == (F, T)
    assert np.array_equal(got, want["llr"].cpu().numpy()) and np.array_equal(got, ref[0])
    assert np.array_equal(np.load(os.path.join(out, "decoded.npy")), want["bits"].cpu().numpy())
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "offset", "status", "distance", "zeros", "weakest", "saturated", "end_state"]
    rec = ref[2]
    assert [[int(x) for x in r] for r in rows[1:]] == \
        [[i, int(offsets[i]), rec[i, 3], rec[i, 0], rec[i, 1], rec[i, 4], rec[i, 5], rec[i, 2]] for i in range(F)]
    assert f"Decoded {F} frames of {T} steps (0 skipped)" in run.stdout

"""cvd_viterbi_decode_frames_list and cvd_frames_crc on the GPU against the sequential references of
list_cases.py, which are written from the text of include/cvd.h: exact equality of every row of
bits, every path record, every frame record and the five totals, at the smallest shapes at which
the kernel can go wrong (S below, at and above a wave; every list width and the truncated ones;
frames with fewer paths than L; frames whose decisions fit the tile in LDS and frames that go
through the workspace, to the largest shape; every boundary condition; inputs that make ties the
rule; every kind of placement; a launch with fewer waves than frames), the identities with
decode_frames_soft that the header states, the CRC over a grid of widths and bit offsets, the
selection of decode_frames_crc, and the decode subcommand's two file layouts."""
import csv
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import list_cases as LS
import llr_cases as LC
from conftest import ROOT

pytestmark = pytest.mark.gpu

CODES = [(1, 2), (3, 2), (6, 2), (7, 2), (8, 2), (6, 3), (8, 3)]


@functools.lru_cache(maxsize=None)
def capture(m, n, T, F, s0, e, kind="noisy", gap=5, lead=3):
    """A soft capture of F frames of T steps, `gap` values of noise between them and `lead` before
    the first, the frames' offsets and the stride (computed once, not written to)."""
    gen = LC.gen_of(m, n)
    rng = np.random.default_rng(7919 * m + 31 * n + T)
    stride = n * T + gap
    soft = rng.integers(-20, 21, lead + F * stride, dtype=np.int8)
    offsets = lead + stride * np.arange(F, dtype=np.int64)
    for o in offsets:
        soft[o:o + n * T] = LC.soft_frame(rng, gen, n, m, T, s0, e, kind)[0]
    soft.setflags(write=False)
    offsets.setflags(write=False)
    return soft, offsets, stride


@functools.lru_cache(maxsize=None)
def reference(m, n, T, F, s0, e, kind, L):
    soft, offsets, _ = capture(m, n, T, F, s0, e, kind)
    ref = LS.reference_batch(LC.gen_of(m, n), n, m, soft, T, L, offsets, s0, e)
    for a in ref[:3]:
        a.setflags(write=False)
    return ref


def assert_equals_reference(res, ref, T, L):
    bits, paths, frames, stats = ref
    F, w = bits.shape[0], (T + 31) // 32
    assert res["bits"].dtype == torch.uint8 and tuple(res["bits"].shape) == (F, L, 4 * w)
    got = res["bits"].cpu().numpy()
    assert np.array_equal(got, bits), np.argwhere(got != bits)[:5]
    for name, col in (("distance", 0), ("start_states", 1), ("end_states", 2)):
        g = res[name].cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, paths[:, :, col]), (name, g, paths[:, :, col])
    assert np.array_equal(res["paths"].cpu().numpy(), frames[:, 0]), (res["paths"], frames[:, 0])
    assert np.array_equal(res["status"].cpu().numpy(), frames[:, 1])
    assert [res["total_distance"], res["decoded"], res["skipped"], res["total_paths"], res["words"]] == stats
    assert (res["T"], res["F"], res["L"]) == (T, F, L)


def run_case(pkg, m, n, T, F, s0, e, L, kind="noisy"):
    soft, offsets, stride = capture(m, n, T, F, s0, e, kind)
    ref = reference(m, n, T, F, s0, e, kind, L)
    res = pkg.decode_frames_list(n, m, LC.gen_of(m, n), soft, T, L, F=F, start=3, stride=stride, start_state=s0,
                                 end_state=e)
    assert_equals_reference(res, ref, T, L)
    return res, ref


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("m,n", CODES)
def test_code_shapes_and_list_widths(pkg, m, n, L):
    run_case(pkg, m, n, 100, 5, 0, 0, L)


@pytest.mark.parametrize("L", [4, 8])
@pytest.mark.parametrize("m,n", [(3, 2), (6, 2), (8, 3)])
def test_frame_lengths(pkg, m, n, L):
    """From one step up: frames with fewer paths than L (both states fixed: min(L, 2^(T-m))), whole
    and ragged words, and 1025 steps."""
    for T in sorted({1, m, m + 1, m + 2, m + 3, 31, 32, 33, 63, 64, 65, 1025}):
        F = 2 if T > 1000 else 3
        res, ref = run_case(pkg, m, n, T, F, 0, None, L)
        if T >= m:
            res, ref = run_case(pkg, m, n, T, F, 0, 0, L)
            assert (ref[2][:, 0] == min(L, 1 << min(T - m, 10))).all()


def tile_steps(pkg, n, m, L):
    """The steps of the tile of decisions in LDS, read off the workspace function: the largest T
    that needs no workspace."""
    ws = pkg.lib().cvd_viterbi_list_workspace_bytes
    T = 1
    while T < LS.MAX_T and ws(n, m, 2 * T, 1, L) == 0:
        T *= 2
    return T


@pytest.mark.parametrize("m,n,L", [(6, 2, 8), (6, 2, 4), (5, 2, 8), (7, 2, 8), (8, 2, 8), (8, 3, 4)])
def test_both_decision_placements(pkg, m, n, L):
    """T at the tile in LDS (no workspace), one step above it (two tiles, one through the
    workspace) and one step above two tiles (three), for S <= 64, 128 and 256."""
    ws = pkg.lib().cvd_viterbi_list_workspace_bytes
    ts = tile_steps(pkg, n, m, L)
    assert ts == 16384 // ((1 << m) * L // 2)
    tile = ts * (1 << m) * L // 2
    for T, tiles in ((ts, 1), (ts + 1, 2), (2 * ts, 2), (2 * ts + 1, 3)):
        assert ws(n, m, T, 3, L) == 3 * (tiles - 1) * tile
        run_case(pkg, m, n, T, 3, 0, 0, L)
        run_case(pkg, m, n, T, 3, None, None, L)


def test_largest_shape(pkg):
    """T = 8192, L = 8, 256 states: 512 tiles per frame, 8 MiB per wave."""
    m, n, T, L = 8, 3, LS.MAX_T, LS.MAX_L
    assert pkg.lib().cvd_viterbi_list_workspace_bytes(n, m, T, 2, L) == 2 * 511 * 16384
    res, ref = run_case(pkg, m, n, T, 2, 0, 0, L)
    assert (ref[2][:, 0] == L).all()


@pytest.mark.parametrize("m,n", [(3, 2), (6, 2), (6, 3), (7, 2), (8, 2)])
def test_boundary_states(pkg, m, n):
    S = 1 << m
    s, e = S - 2, (S // 2) | 1
    for s0, e0 in ((0, 0), (None, None), (s, None), (None, e), (s, e)):
        for L in (3, 8):
            res, ref = run_case(pkg, m, n, 45, 4, s0, e0, L)
            paths = ref[1]
            if s0 is not None:
                assert (paths[:, :, 1] == s0).all()
            if e0 is not None:
                assert (paths[:, :, 2] == e0).all()


@pytest.mark.parametrize("kind", ["noisy", "m128", "zero", "pm1"])
@pytest.mark.parametrize("m,n", [(2, 2), (6, 2), (8, 2)])
def test_inputs(pkg, m, n, kind):
    T = 50
    for s0, e in ((0, 0), (None, None)):
        for L in (2, 8):
            res, ref = run_case(pkg, m, n, T, 4, s0, e, L, kind)
            d = ref[1][:, :, 0]
            if kind == "zero":
                assert not d.any()                                # every path costs nothing: the order is all ties
            if kind == "pm1":
                assert (d[:, 1:] == d[:, :-1]).any()              # equal distances along a list
    if kind == "m128":
        assert (capture(m, n, T, 4, 0, 0, kind)[0] == -128).any()


def test_offsets(pkg):
    """Offset mode: negative offsets and offsets past the end are skipped (zero rows, absent paths,
    {0, 1}), frames overlap and repeat, offsets are odd and unaligned."""
    m, n, T, L = 6, 2, 70, 5
    gen = LC.gen_of(m, n)
    soft = capture(m, n, T, 5, 0, 0)[0]
    N = len(soft)
    offsets = np.array([3, -1, 3 + n * T + 5, N - n * T + 1, 3, 10, 11, -(1 << 40), N - n * T, N, 1 << 40, 77],
                       dtype=np.int64)
    for s0, e in ((0, 0), (None, None)):
        ref = LS.reference_batch(gen, n, m, soft, T, L, offsets, s0, e)
        assert ref[3][1] == 7 and ref[3][2] == 5
        res = pkg.decode_frames_list(n, m, gen, soft, T, L, offsets=offsets, start_state=s0, end_state=e)
        assert_equals_reference(res, ref, T, L)
        skipped = res["status"].cpu().numpy() == 1
        assert not res["bits"].cpu().numpy()[skipped].any() and not res["paths"].cpu().numpy()[skipped].any()
        assert (res["distance"].cpu().numpy()[skipped] == -1).all()
    # a device tensor of offsets, and only skipped frames
    res = pkg.decode_frames_list(n, m, gen, soft, T, L, offsets=torch.tensor([-5, N], dtype=torch.int64, device="cuda"))
    assert_equals_reference(res, LS.reference_batch(gen, n, m, soft, T, L, [-5, N], 0, 0), T, L)


def test_strides(pkg):
    """Stride mode: a stride larger than the frame (capture() has a gap), an odd start, frames
    that follow one another, and overlapping frames at stride 1."""
    m, n, T, L = 5, 2, 37, 4
    gen = LC.gen_of(m, n)
    soft, offsets, stride = capture(m, n, T, 6, 0, None)
    assert stride > n * T and offsets[0] % 2 == 1
    run_case(pkg, m, n, T, 6, 0, None, L)
    for start, st, F in ((0, n * T, 6), (1, 1, 9), (5, 3, None)):
        res = pkg.decode_frames_list(n, m, gen, soft, T, L, F=F, start=start, stride=st, start_state=None, end_state=None)
        off = start + st * np.arange(res["F"])
        assert F is None or res["F"] == F
        assert_equals_reference(res, LS.reference_batch(gen, n, m, soft, T, L, off, None, None), T, L)


@pytest.mark.parametrize("m,n,T", [(4, 2, 100), (6, 2, 100), (8, 2, 100)])
def test_same_result_on_every_launch(pkg, monkeypatch, m, n, T):
    """F = 10 frames on 3 waves and on 1: the grid stride, a wave's slice of the workspace reused
    (m = 6 and 8 at L = 8: two and seven tiles)."""
    F, L = 10, 8
    soft, offsets, stride = capture(m, n, T, F, 0, 0)
    ref = reference(m, n, T, F, 0, 0, "noisy", L)
    gen = LC.gen_of(m, n)
    ws = pkg.lib().cvd_viterbi_list_workspace_bytes
    full = ws(n, m, T, F, L)
    for waves in ("3", "1"):
        monkeypatch.setenv("CVD_LIST_WAVES", waves)
        assert ws(n, m, T, F, L) == full // F * int(waves)
        assert_equals_reference(pkg.decode_frames_list(n, m, gen, soft, T, L, F=F, start=3, stride=stride), ref, T, L)
    monkeypatch.delenv("CVD_LIST_WAVES")
    assert_equals_reference(pkg.decode_frames_list(n, m, gen, soft, T, L, F=F, start=3, stride=stride), ref, T, L)


@pytest.mark.parametrize("kind", ["noisy", "pm1"])
@pytest.mark.parametrize("m,n", [(2, 2), (6, 2), (6, 3), (7, 2), (8, 3)])
def test_path_0_is_decode_frames_soft(pkg, m, n, kind):
    """On the same arguments path 0 is decode_frames_soft's in bits, distance, s_0 and s_T, for
    every L; with L = 1 that is the whole result.  A theorem, so no exception is allowed."""
    T, F = 90, 40
    gen = LC.gen_of(m, n)
    S = 1 << m
    for s0, e in ((0, 0), (None, None), (S - 1, None), (None, 1)):
        rng = np.random.default_rng(100 * m + n)
        soft = np.concatenate([LC.soft_frame(rng, gen, n, m, T, s0, e, kind, sigma=0.9)[0] for _ in range(F)])
        b = pkg.decode_frames_soft(n, m, gen, soft, T, start_state=s0, end_state=e)
        for L in (1, 4, 8):
            a = pkg.decode_frames_list(n, m, gen, soft, T, L, start_state=s0, end_state=e)
            assert a["F"] == b["F"] == F
            assert torch.equal(a["bits"][:, 0], b["bits"])
            assert torch.equal(a["distance"][:, 0], b["distance"])
            assert torch.equal(a["start_states"][:, 0], b["start_states"])
            assert torch.equal(a["end_states"][:, 0], b["end_states"])
            assert a["total_distance"] == b["total_distance"] and a["decoded"] == b["decoded"]
            d = a["distance"].cpu().numpy()
            assert (d[:, 1:] >= d[:, :-1]).all()
            if L == 1:
                assert a["total_paths"] == F and (a["paths"] == 1).all()


CRC_WIDTHS = {1: 0x1, 8: 0x9B, 16: 0x1021, 24: 0x864CFB, 32: 0x04C11DB7}


@pytest.mark.parametrize("width", sorted(CRC_WIDTHS))
def test_frames_crc_grid(pkg, width):
    """Random rows; every first in {0, 1, 31, 32, 33} with every count in {0, 1, 7, 8, 9, 63, 64,
    65, 1000} in the fewest words that hold them, and for every first two counts with which the
    field ends exactly at the row's last bit; init zero and all ones."""
    poly = CRC_WIDTHS[width]
    rng = np.random.default_rng(width)
    firsts, counts = (0, 1, 31, 32, 33), (0, 1, 7, 8, 9, 63, 64, 65, 1000)
    cases = [(f, c) for f in firsts for c in counts]
    cases += [(f, (-(f + width)) % 32 + 32 * k) for f in firsts for k in (0, 2)]      # the field ends exactly at 32 w
    for f, c in cases:
        w = (f + c + width + 31) // 32
        rows = rng.integers(0, 256, (37, 4 * w), dtype=np.uint8)
        init = (1 << width) - 1 if (f + c) % 2 else 0
        got = pkg.frames_crc(rows, f, c, (width, poly, init, 0))
        assert got.dtype == torch.int64 and tuple(got.shape) == (37,)
        want = LS.reference_crc(rows, f, c, width, poly, init)
        assert np.array_equal(got.cpu().numpy(), want), (width, f, c, w)


def test_frames_crc_layouts(pkg):
    """A device tensor with leading dimensions, more rows than a launch's threads stride over in one
    pass would need care for, and the named specs on rows with an appended CRC."""
    rng = np.random.default_rng(5)
    for name, (width, poly, init, expect) in LS.CRC_SPECS.items():
        data = rng.integers(0, 2, (6, 3, 75)).astype(np.uint8)
        rows = np.zeros((6, 3, 128), dtype=np.uint8)
        for i in range(6):
            for j in range(3):
                rows[i, j, 5:5 + 75 + width] = LS.crc_append(data[i, j], width, poly, init, expect)
        rows[1, 2, 40] ^= 1
        bits = torch.from_numpy(LS.pack_rows(rows, 4)).cuda()
        got = pkg.frames_crc(bits, 5, 75, name)
        assert got.is_cuda and tuple(got.shape) == (6, 3)
        ok = got.cpu().numpy() == expect
        assert ok.sum() == 17 and not ok[1, 2]
        assert np.array_equal(got.cpu().numpy(), LS.reference_crc(LS.pack_rows(rows, 4), 5, 75, width, poly, init))
    many = rng.integers(0, 256, (70001, 8), dtype=np.uint8)
    got = pkg.frames_crc(many, 3, 40, "crc16-ccitt").cpu().numpy()
    idx = np.r_[0:50, 69950:70001, rng.integers(0, 70001, 200)]
    assert np.array_equal(got[idx], LS.reference_crc(many[idx], 3, 40, 16, 0x1021, 0))
    assert tuple(pkg.frames_crc(np.zeros((0, 8), dtype=np.uint8), 0, 8, "crc8-lte").shape) == (0,)


@functools.lru_cache(maxsize=None)
def crc_case():
    """48 frames of 100 data bits || crc16-ccitt || 6 tail bits of (133,171) at amplitude 32 and
    sigma = 0.9: chosen on the CPU with the reference so that path 0 fails the CRC on some frames
    and a later path passes on some of them (seed 2024: five frames fail, six are rescued)."""
    m, n, F, L = 6, 2, 48, 4
    gen = LC.gen_of(m, n)
    soft, sent, T = LS.crc_frames(np.random.default_rng(2024), gen, n, m, F, 100, "crc16-ccitt", 32, 0.9)
    bits, paths, frames, stats = LS.reference_batch(gen, n, m, soft, T, L, n * T * np.arange(F), 0, 0)
    value = LS.reference_crc(bits, 0, 100, 16, 0x1021, 0)
    choice = LS.select(value, np.arange(L)[None, :] < frames[:, :1], 0)
    return m, n, F, L, T, soft, sent, (bits, paths, frames, stats), value, choice


def test_decode_frames_crc(pkg):
    m, n, F, L, T, soft, sent, ref, value, choice = crc_case()
    bits, paths = ref[0], ref[1]
    assert (choice > 0).sum() > 0 and (choice < 0).sum() > 0
    res = pkg.decode_frames_crc(n, m, LC.gen_of(m, n), soft, T, L, "crc16-ccitt")
    assert_equals_reference(res, ref, T, L)
    assert np.array_equal(res["value"].cpu().numpy(), value)
    assert res["choice"].dtype == torch.int32 and np.array_equal(res["choice"].cpu().numpy(), choice)
    assert np.array_equal(res["crc_ok"].cpu().numpy(), choice >= 0)
    pick = np.maximum(choice, 0)
    assert np.array_equal(res["chosen_bits"].cpu().numpy(), bits[np.arange(F), pick])
    assert np.array_equal(res["chosen_distance"].cpu().numpy(), paths[np.arange(F), pick, 0])
    assert res["ok"] == int((choice >= 0).sum()) and res["rescued"] == int((choice > 0).sum()) > 0
    # the spec, first, count and expect spelt out
    again = pkg.decode_frames_crc(n, m, LC.gen_of(m, n), soft, T, L, "16:1021", first=0, count=100, expect=0)
    assert torch.equal(again["choice"], res["choice"])
    masked = pkg.decode_frames_crc(n, m, LC.gen_of(m, n), soft, T, L, "crc16-ccitt", expect=0x1234)
    assert np.array_equal(masked["choice"].cpu().numpy(),
                          LS.select(value, np.arange(L)[None, :] < ref[2][:, :1], 0x1234))


def test_argument_errors(pkg):
    gen = LC.gen_of(6, 2)
    soft = np.zeros(1000, dtype=np.int8)
    with pytest.raises(ValueError):
        pkg.decode_frames_list(2, 6, gen, soft, 5, 4)              # both states fixed and T < m
    with pytest.raises(ValueError):
        pkg.decode_frames_list(2, 6, gen, soft, 100, 4, F=6)
    with pytest.raises(pkg.CvdError, match="viterbi_decode_frames_list"):
        pkg.decode_frames_list(2, 9, [[[1] * 10], [[1, 0, 1, 1, 1, 0, 0, 0, 1, 1]]], soft, 100, 4)
    res = pkg.decode_frames_list(2, 6, gen, soft, 100, 3, F=0)
    assert res["F"] == 0 and tuple(res["bits"].shape) == (0, 3, 16) and res["decoded"] == 0 and res["words"] == 4


def run_cli(pkg, args):
    pkg_name = os.path.basename(os.path.dirname(pkg.__file__))
    run = subprocess.run([sys.executable, "-m", pkg_name, "decode", "--code", "oct:133,171", "--format", "soft"] + args,
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def test_decode_cli_list(pkg, tmp_path):
    """decode --frame T --format soft --list L in a fresh process: decoded.npy [F, L, 4w] and a CSV
    row per (frame, path)."""
    m, n, T, F, L = 6, 2, 70, 6, 3
    soft, offsets, stride = capture(m, n, T, F, 0, 0)
    bits, paths, frames, stats = reference(m, n, T, F, 0, 0, "noisy", L)
    npy, out = str(tmp_path / "cap.npy"), str(tmp_path / "res")
    np.save(npy, soft)
    stdout = run_cli(pkg, ["--input", npy, "--start", "3", "--frame", str(T), "--frame-stride", str(stride), "--list",
                           str(L), "--save-dir", out])
    got = np.load(os.path.join(out, "decoded.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, bits)
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "path", "offset", "status", "distance", "start_state", "end_state"]
    assert [[int(x) for x in r] for r in rows[1:]] == \
        [[i, l, int(offsets[i]), 0] + paths[i, l].tolist() for i in range(F) for l in range(L)]
    assert f"Decoded {F} frames of {T} steps (0 skipped)" in stdout


def test_decode_cli_crc(pkg, tmp_path):
    """... with --crc: decoded.npy is the chosen rows [F, 4w] and the CSV has a row per frame."""
    m, n, F, L, T, soft, sent, ref, value, choice = crc_case()
    bits, paths, frames, stats = ref
    npy, out = str(tmp_path / "cap.npy"), str(tmp_path / "res")
    np.save(npy, soft)
    stdout = run_cli(pkg, ["--input", npy, "--frame", str(T), "--list", str(L), "--crc", "crc16-ccitt", "--save-dir", out])
    pick = np.maximum(choice, 0)
    got = np.load(os.path.join(out, "decoded.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, bits[np.arange(F), pick])
    with open(os.path.join(out, "decode_frames.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "offset", "status", "paths", "choice", "crc_ok", "distance", "distance0", "start_state",
                       "end_state"]
    want = [[i, n * T * i, 0, int(frames[i, 0]), int(choice[i]), int(choice[i] >= 0), int(paths[i, pick[i], 0]),
             int(paths[i, 0, 0]), int(paths[i, pick[i], 1]), int(paths[i, pick[i], 2])] for i in range(F)]
    assert [[int(x) for x in r] for r in rows[1:]] == want
    assert f"{F} decoded, {int((choice >= 0).sum())} ok, {int((choice > 0).sum())} rescued" in stdout

"""cvd_viterbi_decode_frames_tailbiting_list on the GPU against the sequential reference of
tblist_cases.py, which is written from the text of include/cvd.h: exact equality of every row of
bits, every path record, every frame record and the eight totals, at the smallest shapes at which
the kernel can go wrong (S below, at and above a wave; every list width and the cut ones; frame
lengths from one step over T < m to ragged words; frames whose decisions fit the tile in LDS and
frames that go through the workspace in both traces; every lap limit on inputs that end in every
status; inputs that make ties the rule; every kind of placement; launches with fewer waves than
frames), the identities with decode_frames_tailbiting_soft that the header states, and the CRC
selection of decode_frames_tailbiting_crc."""
import functools

import numpy as np
import pytest
import torch

import list_cases as LS
import llr_cases as LC
import tblist_cases as TB

pytestmark = pytest.mark.gpu

CODES = [(1, 2), (2, 2), (5, 2), (6, 2), (6, 3), (7, 2), (8, 2), (8, 3)]


@functools.lru_cache(maxsize=None)
def capture(m, n, T, F, kind="noisy", gap=5, lead=3):
    """A soft capture of F frames of T steps, `gap` values of noise between them and `lead` before
    the first, the frames' offsets and the stride (computed once, not written to).  "noisy": tail-
    biting frames at amplitude 24, sigma = 1.35; the other kinds are llr_cases.soft_frame's."""
    gen = LC.gen_of(m, n)
    rng = np.random.default_rng(7919 * m + 31 * n + T)
    stride = n * T + gap
    soft = rng.integers(-20, 21, lead + F * stride, dtype=np.int8)
    offsets = lead + stride * np.arange(F, dtype=np.int64)
    for o in offsets:
        if kind == "noisy":
            soft[o:o + n * T] = TB.tailbiting_frames(rng, gen, n, m, 1, T, 24, 1.35)[0]
        else:
            soft[o:o + n * T] = LC.soft_frame(rng, gen, n, m, T, None, None, kind)[0]
    soft.setflags(write=False)
    offsets.setflags(write=False)
    return soft, offsets, stride


@functools.lru_cache(maxsize=None)
def reference(m, n, T, F, kind, L, laps=TB.DEFAULT_LAPS):
    soft, offsets, _ = capture(m, n, T, F, kind)
    ref = TB.reference_batch(LC.gen_of(m, n), n, m, soft, T, L, offsets, laps)
    for a in ref[:3]:
        a.setflags(write=False)
    return ref


def assert_equals_reference(res, ref, T, L):
    bits, paths, frames, stats = ref[:4]
    F, w = bits.shape[0], (T + 31) // 32
    assert res["bits"].dtype == torch.uint8 and tuple(res["bits"].shape) == (F, L, 4 * w)
    got_frames = res["frames"].cpu().numpy()
    assert got_frames.dtype == np.int32 and np.array_equal(got_frames, frames), \
        (np.argwhere(got_frames != frames)[:5], got_frames[:4], frames[:4])
    for name, col in (("distance", 0), ("start_states", 1), ("end_states", 2)):
        g = res[name].cpu().numpy()
        assert g.dtype == np.int32 and np.array_equal(g, paths[:, :, col]), \
            (name, np.argwhere(g != paths[:, :, col])[:5])
    got = res["bits"].cpu().numpy()
    assert np.array_equal(got, bits), np.argwhere(got != bits)[:5]
    for name, col in (("paths", 0), ("status", 1), ("laps", 2), ("candidates", 3)):
        assert np.array_equal(res[name].cpu().numpy(), frames[:, col]), name
    assert [res["total_distance"], res["decoded"], res["skipped"], res["total_paths"], res["words"], res["fallback"],
            res["open"], res["total_laps"]] == stats
    assert (res["T"], res["F"], res["L"]) == (T, F, L)


def run_case(pkg, m, n, T, F, L, kind="noisy", laps=None):
    soft, offsets, stride = capture(m, n, T, F, kind)
    ref = reference(m, n, T, F, kind, L, TB.DEFAULT_LAPS if laps is None else laps)
    res = pkg.decode_frames_tailbiting_list(n, m, LC.gen_of(m, n), soft, T, L, F=F, start=3, stride=stride, max_laps=laps)
    assert_equals_reference(res, ref, T, L)
    return res, ref


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("m,n", CODES)
def test_code_shapes_and_list_widths(pkg, m, n, L):
    res, ref = run_case(pkg, m, n, 40, 70, L)
    if m >= 5:
        assert len(set(ref[2][:, 2].tolist())) > 1           # more than one number of laps


@pytest.mark.parametrize("L", [3, 8])
@pytest.mark.parametrize("m,n", [(2, 2), (6, 2), (8, 3)])
def test_frame_lengths(pkg, m, n, L):
    """From one step up, T < m included (the state wraps more than once), whole and ragged words."""
    for T in sorted({1, 2, m - 1, m, m + 1, 31, 32, 33, 63, 64, 65, 129}):
        run_case(pkg, m, n, T, 4, L)


@pytest.mark.parametrize("m,n,L,lds", [(6, 2, 4, 1024), (5, 2, 2, 1024), (6, 3, 8, 2048), (8, 2, 8, 4096), (8, 3, 3, 2048)])
def test_decision_placements(pkg, monkeypatch, m, n, L, lds):
    """With a small tile: T one step below the tile, at it (no workspace), one step above (two
    tiles), at two tiles and one step above them (three), and 40 steps (many): both traces bring
    the tiles back through the workspace, lap after lap."""
    monkeypatch.setenv("CVD_LIST_LDS_BYTES", str(lds))
    ws = pkg.lib().cvd_viterbi_tailbiting_list_workspace_bytes
    LL = 2 if L <= 2 else 4 if L <= 4 else 8
    step = (1 << m) * LL // 2
    ts = lds // step
    assert ts >= 2
    for T in sorted({ts - 1, ts, ts + 1, 2 * ts, 2 * ts + 1, 40}):
        assert ws(n, m, T, 5, L) == 5 * ((T + ts - 1) // ts - 1) * ts * step
        res, ref = run_case(pkg, m, n, T, 5, L)
    assert (ref[2][:, 2] > 1).any()                          # T = 40: frames that go round more than once


@pytest.mark.parametrize("laps", [1, 2, 4, 8])
@pytest.mark.parametrize("i", range(len(TB.COVERING)))
def test_laps_on_the_covering_inputs(pkg, i, laps):
    """The inputs that tests/test_decode_tblist_host.py shows to end in every status, after every
    number of laps and by the repeat of E, with fewer paths than L and with L of them."""
    m, n, T, F, sigma, seed = TB.COVERING[i]
    gen, soft = TB.covering_capture(m, n, T, F, sigma, seed)
    for L in (4, 8) if laps == TB.DEFAULT_LAPS else (4,):
        res = pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L, max_laps=laps)
        assert_equals_reference(res, TB.covering_reference(i, L, laps), T, L)
    if laps == TB.DEFAULT_LAPS:
        again = pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, 4)      # the default is 4 laps
        assert_equals_reference(again, TB.covering_reference(i, 4, laps), T, 4)


@pytest.mark.parametrize("kind", ["m128", "zero", "pm1"])
@pytest.mark.parametrize("m,n", [(2, 2), (6, 2), (8, 2)])
def test_inputs(pkg, m, n, kind):
    T = 40
    for L in (2, 8):
        res, ref = run_case(pkg, m, n, T, 4, L, kind)
        if kind == "zero":                                    # every path costs nothing: the order is all ties
            assert not ref[1][:, :, 0].any() and (ref[2][:, 1] == 0).all() and (ref[2][:, 0] == L).all()
    if kind == "m128":
        assert (capture(m, n, T, 4, kind)[0] == -128).any()


def test_offsets(pkg):
    """Offset mode: negative offsets and offsets past the end are skipped (zero rows, absent paths,
    {0, 1, 0, 0}), frames overlap and repeat, offsets are odd and unaligned."""
    m, n, T, L = 6, 2, 40, 5
    gen = LC.gen_of(m, n)
    soft = capture(m, n, T, 5)[0]
    N = len(soft)
    offsets = np.array([3, -1, 3 + n * T + 5, N - n * T + 1, 3, 10, 11, -(1 << 40), N - n * T, N, 1 << 40, 77],
                       dtype=np.int64)
    ref = TB.reference_batch(gen, n, m, soft, T, L, offsets)
    assert ref[3][1] == 7 and ref[3][2] == 5
    res = pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L, offsets=offsets)
    assert_equals_reference(res, ref, T, L)
    skipped = res["status"].cpu().numpy() == 1
    assert not res["bits"].cpu().numpy()[skipped].any() and (res["distance"].cpu().numpy()[skipped] == -1).all()
    # a device tensor of offsets, and only skipped frames
    res = pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L,
                                            offsets=torch.tensor([-5, N], dtype=torch.int64, device="cuda"))
    assert_equals_reference(res, TB.reference_batch(gen, n, m, soft, T, L, [-5, N]), T, L)


def test_strides(pkg):
    """Stride mode: a stride larger than the frame (capture() has a gap), an odd start, frames
    that follow one another, and overlapping frames at stride 1."""
    m, n, T, L = 5, 2, 37, 4
    gen = LC.gen_of(m, n)
    soft, offsets, stride = capture(m, n, T, 6)
    assert stride > n * T and offsets[0] % 2 == 1
    run_case(pkg, m, n, T, 6, L)
    for start, st, F in ((0, n * T, 6), (1, 1, 9), (5, 3, None)):
        res = pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L, F=F, start=start, stride=st)
        off = start + st * np.arange(res["F"])
        assert F is None or res["F"] == F
        assert_equals_reference(res, TB.reference_batch(gen, n, m, soft, T, L, off), T, L)


@pytest.mark.parametrize("m,n,T", [(4, 2, 40), (6, 2, 100), (8, 2, 40)])
def test_same_result_on_every_launch(pkg, monkeypatch, m, n, T):
    """F = 10 frames on 3 waves and on 1: the grid stride, a wave's slice of the workspace reused
    frame after frame and lap after lap (m = 6 and 8 at L = 8: two and three tiles)."""
    F, L = 10, 8
    soft, offsets, stride = capture(m, n, T, F)
    ref = reference(m, n, T, F, "noisy", L)
    gen = LC.gen_of(m, n)
    ws = pkg.lib().cvd_viterbi_tailbiting_list_workspace_bytes
    full = ws(n, m, T, F, L)
    assert (full > 0) == (m >= 6)
    for waves in ("3", "1"):
        monkeypatch.setenv("CVD_LIST_WAVES", waves)
        assert ws(n, m, T, F, L) == full // F * int(waves)
        assert_equals_reference(pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L, F=F, start=3, stride=stride),
                                ref, T, L)
    monkeypatch.delenv("CVD_LIST_WAVES")
    assert_equals_reference(pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L, F=F, start=3, stride=stride), ref,
                            T, L)


@pytest.mark.parametrize("i", range(len(TB.COVERING)))
def test_sibling_consistency(pkg, i):
    """L = 1 is decode_frames_tailbiting_soft field by field, and path 0 is at L = 8.  A theorem,
    so no exception is allowed."""
    m, n, T, F, sigma, seed = TB.COVERING[i]
    gen, soft = TB.covering_capture(m, n, T, F, sigma, seed)
    for laps in (None, 1, 8):
        b = pkg.decode_frames_tailbiting_soft(n, m, gen, soft, T, max_laps=laps)
        for L in (1, 8):
            a = pkg.decode_frames_tailbiting_list(n, m, gen, soft, T, L, max_laps=laps)
            assert a["F"] == b["F"] == F
            assert torch.equal(a["bits"][:, 0], b["bits"])
            assert torch.equal(a["distance"][:, 0], b["distance"])
            assert torch.equal(a["start_states"][:, 0], b["start_states"])
            assert torch.equal(a["end_states"][:, 0], b["end_states"])
            assert torch.equal(a["status"], b["status"]) and torch.equal(a["laps"], b["laps"])
            assert (a["total_distance"], a["decoded"], a["skipped"], a["fallback"], a["open"], a["total_laps"]) == \
                (b["total_distance"], b["decoded"], b["skipped"], b["fallback"], b["open"], b["total_laps"])
            if L == 1:
                assert a["total_paths"] == F and (a["paths"] == 1).all()


@functools.lru_cache(maxsize=None)
def crc_case(sigma, mask=0):
    """96 LTE-PBCH-shaped frames: 24 data bits || crc16-ccitt ^ mask, tail-biting (133,171,165), at
    amplitude 24, with the reference's list of 4, CRC values and choice."""
    m, n, F, L = 6, 3, 96, 4
    gen = LC.gen_of(m, n)
    soft, sent, T = TB.crc_frames(np.random.default_rng(2025), gen, n, m, F, 24, "crc16-ccitt", 24, sigma, mask)
    ref = TB.reference_batch(gen, n, m, soft, T, L, n * T * np.arange(F))
    value = LS.reference_crc(ref[0], 0, 24, 16, 0x1021, 0)
    choice = LS.select(value, np.arange(L)[None, :] < ref[2][:, :1], mask)
    return m, n, F, L, T, gen, soft, sent, ref, value, choice


def test_decode_frames_tailbiting_crc_noise_free(pkg):
    m, n, F, L, T, gen, soft, sent, ref, value, choice = crc_case(0.0)
    res = pkg.decode_frames_tailbiting_crc(n, m, gen, soft, T, L, "crc16-ccitt")
    assert_equals_reference(res, ref, T, L)
    assert (res["choice"] == 0).all() and res["crc_ok"].all() and res["ok"] == F and res["rescued"] == 0
    assert np.array_equal(LS.unpack_rows(res["chosen_bits"].cpu().numpy())[:, :T], sent)
    assert not res["chosen_distance"].any()


def test_decode_frames_tailbiting_crc_noisy(pkg):
    m, n, F, L, T, gen, soft, sent, ref, value, choice = crc_case(1.1)
    bits, paths = ref[0], ref[1]
    assert (choice > 0).sum() > 0 and (choice < 0).sum() > 0
    res = pkg.decode_frames_tailbiting_crc(n, m, gen, soft, T, L, "crc16-ccitt")
    assert_equals_reference(res, ref, T, L)
    assert np.array_equal(res["value"].cpu().numpy(), value)
    assert res["choice"].dtype == torch.int32 and np.array_equal(res["choice"].cpu().numpy(), choice)
    assert np.array_equal(res["crc_ok"].cpu().numpy(), choice >= 0)
    pick = np.maximum(choice, 0)
    assert np.array_equal(res["chosen_bits"].cpu().numpy(), bits[np.arange(F), pick])
    assert np.array_equal(res["chosen_distance"].cpu().numpy(), paths[np.arange(F), pick, 0])
    assert res["ok"] == int((choice >= 0).sum()) and res["rescued"] == int((choice > 0).sum()) > 0
    # the spec, first, count and expect spelt out
    again = pkg.decode_frames_tailbiting_crc(n, m, gen, soft, T, L, "16:1021", first=0, count=24, expect=0)
    assert torch.equal(again["choice"], res["choice"])


def test_decode_frames_tailbiting_crc_rnti(pkg):
    """A CRC masked with an RNTI: with expect=None the identity is read out of value; with
    expect=RNTI the selection is the reference's."""
    rnti = 0xBEEF
    m, n, F, L, T, gen, soft, sent, ref, value, choice = crc_case(1.1, rnti)
    res = pkg.decode_frames_tailbiting_crc(n, m, gen, soft, T, L, "crc16-ccitt")
    assert np.array_equal(res["value"].cpu().numpy(), value)
    right = (LS.unpack_rows(ref[0][:, 0])[:, :T] == sent).all(axis=1)
    assert right.sum() > F // 2 and (res["value"].cpu().numpy()[right, 0] == rnti).all()
    res = pkg.decode_frames_tailbiting_crc(n, m, gen, soft, T, L, "crc16-ccitt", expect=rnti)
    assert np.array_equal(res["choice"].cpu().numpy(), choice) and res["rescued"] == int((choice > 0).sum())


def test_argument_errors(pkg):
    gen = LC.gen_of(6, 2)
    soft = np.zeros(1000, dtype=np.int8)
    with pytest.raises(ValueError):
        pkg.decode_frames_tailbiting_list(2, 6, gen, soft, 100, 4, F=6)
    with pytest.raises(pkg.CvdError, match="viterbi_decode_frames_tailbiting_list"):
        pkg.decode_frames_tailbiting_list(2, 9, [[[1] * 10], [[1, 0, 1, 1, 1, 0, 0, 0, 1, 1]]], soft, 100, 4)
    res = pkg.decode_frames_tailbiting_list(2, 6, gen, soft, 100, 3, F=0)
    assert res["F"] == 0 and tuple(res["bits"].shape) == (0, 3, 16) and res["decoded"] == 0 and res["words"] == 4

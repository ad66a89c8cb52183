"""cvd_viterbi_decode_frames_tailbiting_list without a GPU: the two reference decoders of
tblist_cases.py agree; they satisfy the consequences that include/cvd.h states (L = 1 is the
tail-biting decoder, rows are distinct, paths from 1 on are tail-biting and ordered) and the two
non-consequences are pinned on fixed frames (L = 3 is not L = 4 cut to three; path 1 can be
cheaper than path 0); the inputs of the GPU tests cover every outcome of the rule; every
invalid-argument case of the entry returning CVD_E_INVALID with the entry's name before the device
is touched (the pointers here are never dereferenced); the unsupported shapes; F == 0; the
workspace size under the two environment variables; the exports; the wrappers' refusals."""
import importlib
import os
import re

import numpy as np
import pytest

import list_cases as LS
import llr_cases as LC
import tblist_cases as TB
import test_gpu_decode_tailbite as TG
from conftest import ROOT

I64_MAX = (1 << 63) - 1
GIB = 1 << 30
M6 = LC.gen_of(6, 2)
NAME = b"viterbi_decode_frames_tailbiting_list"

# a valid call of (133,171): five frames of 100 steps from value 3, the last one ending at nvals.
# It is only ever sent with F = 0 or with one argument spoilt: nothing here launches.
GOOD = dict(cap=0x10000, nvals=3 + 5 * 200, start=3, stride=200, offsets=None, F=5, T=100, laps=0, L=4,
            bits=0x20000, paths=0x70000, frames=0x50000, stats=0x30000, work=0x40000)


def call(pkg, code=None, **kw):
    a = dict(GOOD, **kw)
    code = pkg.Code(M6, 6, 1, 2) if code is None else code
    return pkg.lib().cvd_viterbi_decode_frames_tailbiting_list(code.c, a["cap"], a["nvals"], a["start"], a["stride"],
                                                               a["offsets"], a["F"], a["T"], a["laps"], a["L"], a["bits"],
                                                               a["paths"], a["frames"], a["stats"], a["work"], None)


def key(paths):
    return [(p[0], p[1].tolist(), p[2], p[3]) for p in paths]


# ── the two references, and the contract's consequences on them ──

covering = TB.covering_reference


def test_the_two_references_agree():
    for m, n, T, F, kind in ((1, 2, 5, 12, "noisy"), (2, 2, 1, 8, "noisy"), (2, 2, 7, 12, "pm1"), (3, 2, 12, 30, "noisy"),
                             (3, 2, 2, 8, "zero"), (6, 3, 9, 3, "noisy")):
        gen = LC.gen_of(m, n)
        rng = np.random.default_rng(100 * m + T)
        for f in range(F):
            if kind == "noisy":
                v = TB.tailbiting_frames(rng, gen, n, m, 1, T, 24, 1.4)[0]
            else:
                v = LC.soft_frame(rng, gen, n, m, T, None, None, kind)[0]
            for L in (1, 2, 3, 4, 5, 8):
                for laps in (1, 4):
                    a = TB.tblist_frame_plain(gen, n, m, v, T, L, laps)
                    b = TB.tblist_frame(gen, n, m, v, T, L, laps)
                    assert key(a[0]) == key(b[0]) and a[1:] == b[1:], (m, n, T, f, L, laps)


@pytest.mark.parametrize("i", range(len(TB.COVERING)))
def test_reference_satisfies_the_contract(i):
    m, n, T, F, sigma, seed = TB.COVERING[i]
    gen, soft = TB.covering_capture(m, n, T, F, sigma, seed)
    out = LC.branch_outputs(gen, n, m)
    # L = 1 is the tail-biting decoder's reference, written independently (tests/test_gpu_decode_tailbite.py)
    v = soft.reshape(F, T, n)
    tb_bits, tb_rec, _, tb_rep = TG.ref_tailbiting(n, m, gen, TG.soft_cost(n, v), TB.DEFAULT_LAPS)
    bits, paths, frames, stats, rep = covering(i, 1)
    assert np.array_equal(bits[:, 0], TG.pack_rows(tb_bits))
    assert np.array_equal(paths[:, 0], tb_rec[:, :3]) and np.array_equal(frames[:, 1], tb_rec[:, 3])
    assert np.array_equal(frames[:, 2], tb_rec[:, 6]) and np.array_equal(rep, tb_rep) and (frames[:, 0] == 1).all()
    for L in (2, 3, 4, 8):
        b, p, fr, st, _ = covering(i, L)
        # path 0, status and laps do not depend on L
        assert np.array_equal(b[:, 0], bits[:, 0]) and np.array_equal(p[:, 0], paths[:, 0])
        assert np.array_equal(fr[:, 1:3], frames[:, 1:3])
        u = LS.unpack_rows(b)[:, :, :T]
        for f in range(F):
            P, status, laps, nC = fr[f]
            assert P == 1 + min(L - 1, nC - (status != 3))
            assert (p[f, P:] == -1).all() and not b[f, P:].any()
            c, s0, sT = p[f, :P, 0], p[f, :P, 1], p[f, :P, 2]
            assert (s0[1:] == sT[1:]).all()                    # paths from 1 on are tail-biting
            assert (s0[0] == sT[0]) == (status != 3)
            assert (np.diff(c[1:]) >= 0).all()                 # ordered from 1 on
            first = 0 if status != 3 else 1                    # distinct rows, a tail-biting path 0 among them
            assert len({u[f, l].tobytes() for l in range(first, P)}) == P - first
            cost = LC.step_costs(soft[f * n * T:(f + 1) * n * T], n, T)
            for l in range(P):                                 # every path is a path: its bits give its cost and its end
                s, tot = int(s0[l]), 0
                for t in range(T):
                    tot += int(cost[t][out[s, int(u[f, l, t])]])
                    s = ((s << 1) | int(u[f, l, t])) & ((1 << m) - 1)
                assert (tot, s) == (c[l], sT[l])
        ok = fr[:, 1] != 1
        assert st == [int(p[ok, 0, 0].sum()), F, 0, int(fr[:, 0].sum()), (T + 31) // 32, int((fr[:, 1] == 2).sum()),
                      int((fr[:, 1] == 3).sum()), int(fr[:, 2].sum())]


def test_the_result_for_L_is_not_a_prefix():
    """Frame 36 of the (15,17) input (status 0): the three paths of L = 3 are not the first three
    of L = 4, whose third is cheaper than the third of L = 3."""
    m, n, T, F, sigma, seed = TB.COVERING[2]
    gen, soft = TB.covering_capture(m, n, T, F, sigma, seed)
    v = soft[36 * n * T:37 * n * T]
    a3, a4 = TB.tblist_frame(gen, n, m, v, T, 3), TB.tblist_frame(gen, n, m, v, T, 4)
    assert len(a3[0]) == 3 and len(a4[0]) == 4
    assert key(a3[0]) != key(a4[0][:3]) and a4[0][2][0] < a3[0][2][0]
    assert key(a3[0])[0] == key(a4[0])[0]                      # path 0 is the same
    assert key(TB.tblist_frame_plain(gen, n, m, v, T, 3)[0]) == key(a3[0])


def test_path_1_can_be_cheaper_than_path_0():
    """Frame 34 of the (15,17) input: status 2 or 3, and path 1 costs less than path 0."""
    m, n, T, F, sigma, seed = TB.COVERING[2]
    gen, soft = TB.covering_capture(m, n, T, F, sigma, seed)
    paths, status, laps, nC, _ = TB.tblist_frame_plain(gen, n, m, soft[34 * n * T:35 * n * T], T, 3)
    assert status in (2, 3) and paths[1][0] < paths[0][0] and paths[1][2] == paths[1][3]


@pytest.mark.parametrize("i", range(len(TB.COVERING)))
def test_gpu_inputs_cover_the_outcomes(i):
    I = TB.DEFAULT_LAPS
    for L in (4, 8):
        bits, paths, frames, stats, rep = covering(i, L)
        P, status, laps = frames[:, 0], frames[:, 1], frames[:, 2]
        for s in (0, 2, 3):
            assert (status == s).sum() >= 5, (L, s)
        for l in range(1, I + 1):
            assert (laps == l).sum() >= 5, (L, l)
        assert rep.sum() >= 5 and (laps[rep] < I).all() and (laps[rep] >= 2).all()
        assert (P < L).sum() >= 5 and (P == L).sum() >= 5
        assert ((status == 3) & (P > 1)).sum() >= 5
        assert ((status == 0) & (laps == 1)).any() and ((status != 0) & (laps == I)).any()
    # the other lap limits end in every status too
    for laps in (1, 2, 8):
        fr = covering(i, 4, laps)[2]
        assert (fr[:, 2] <= laps).all() and (fr[:, 2] == min(laps, 2)).any()
        assert all((fr[:, 1] == s).any() for s in (0, 2, 3))


def test_reference_batch_records():
    gen, rng = LC.gen_of(3, 2), np.random.default_rng(9)
    T, L = 5, 8
    soft, _ = TB.tailbiting_frames(rng, gen, 2, 3, 2, T)
    bits, paths, frames, stats, rep = TB.reference_batch(gen, 2, 3, soft, T, L, [0, -1, 10, 11], 4)
    assert bits.shape == (4, L, 4) and paths.shape == (4, L, 3) and frames.shape == (4, 4)
    assert frames[1].tolist() == frames[3].tolist() == TB.SKIPPED
    assert (paths[1] == -1).all() and not bits[1].any()
    assert stats[:5] == [int(paths[0, 0, 0] + paths[2, 0, 0]), 2, 2, int(frames[:, 0].sum()), 1]
    assert stats[7] == int(frames[:, 2].sum())


def test_circular_encoder_and_crc_frames():
    gen = LC.gen_of(6, 3)
    rng = np.random.default_rng(4)
    soft, sent, T = TB.crc_frames(rng, gen, 3, 6, 6, 24, "crc16-ccitt", 24, 0.0, mask=0xBEEF)
    assert T == 40 and soft.shape == (6 * 3 * 40,)
    for f in range(6):
        assert LS.crc_value(sent[f], 0, 24, 16, 0x1021) == 0xBEEF
        paths, status, laps, nC, _ = TB.tblist_frame(gen, 3, 6, soft[f * 120:(f + 1) * 120], T, 2)
        assert status == 0 and paths[0][0] == 0 and np.array_equal(paths[0][1], sent[f])
        assert paths[0][2] == paths[0][3] == TG.wrap_state(6, sent[f:f + 1].astype(np.int64))[0]


# ── the library's argument checks ──

INVALID = {
    "T_zero": dict(T=0),
    "T_negative": dict(T=-1),
    "T_above_max": dict(T=8193, nvals=I64_MAX, stride=1 << 20),
    "L_zero": dict(L=0),
    "L_negative": dict(L=-1),
    "L_above_max": dict(L=9),
    "laps_negative": dict(laps=-1),
    "laps_nine": dict(laps=9),
    "F_negative": dict(F=-1),
    "F_times_L_times_w_is_2_31": dict(T=32, L=8, F=1 << 28, stride=1, nvals=I64_MAX),
    "F_times_L_times_w_above_2_31": dict(T=33, L=3, F=1 << 29, stride=1, nvals=I64_MAX),
    "start_negative": dict(start=-1),
    "stride_zero": dict(stride=0),
    "stride_negative": dict(stride=-200),
    "last_frame_one_past_nvals": dict(nvals=GOOD["nvals"] - 1),
    "start_pushes_last_frame_out": dict(start=4),
    "one_frame_more": dict(F=6),
    "start_overflows": dict(start=I64_MAX - 100, nvals=I64_MAX),
    "stride_product_overflows": dict(stride=I64_MAX // 2, nvals=I64_MAX),
    "nvals_negative": dict(nvals=-1),
    "null_capture": dict(cap=None),
    "null_bits": dict(bits=None),
    "null_paths": dict(paths=None),
    "null_frames": dict(frames=None),
    "null_stats": dict(stats=None),
    "null_work_where_one_is_needed": dict(T=300, nvals=3 + 5 * 600, stride=600, L=8, work=None),
    "misaligned_capture": dict(cap=0x10008),
    "misaligned_work": dict(work=0x40008),
    "misaligned_bits": dict(bits=0x20002),
    "misaligned_paths": dict(paths=0x70002),
    "misaligned_frames": dict(frames=0x50002),
    "misaligned_stats": dict(stats=0x30004),
    "misaligned_offsets": dict(offsets=0x60004),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments(pkg, monkeypatch, case):
    monkeypatch.delenv("CVD_LIST_LDS_BYTES", raising=False)
    assert call(pkg, F=0) == 0             # the base arguments themselves are valid
    rc = call(pkg, **INVALID[case])
    assert rc == -1, (case, rc)
    msg = pkg.lib().cvd_last_error()
    assert msg and msg.startswith(NAME + b":"), (case, msg)


def test_no_frames_is_ok_without_a_launch(pkg):
    null = dict(cap=None, bits=None, paths=None, frames=None, stats=None, work=None)
    for laps in (0, 1, 4, 8):
        for L in (1, 8):
            assert call(pkg, F=0, laps=laps, L=L, **null) == 0
    assert call(pkg, F=0, nvals=0, start=0, **null) == 0
    assert call(pkg, F=0, T=0, **null) == 0              # T is a property of the frames
    assert call(pkg, F=0, T=8193, **null) == 0
    assert call(pkg, F=0, T=3, **null) == 0              # T < m is allowed
    assert call(pkg, F=0, offsets=0x60000, start=-5, stride=0, **null) == 0      # offset mode ignores both
    assert call(pkg, F=0, L=9, **null) == -1             # the arguments are still checked


def test_unsupported_shapes(pkg):
    lib = pkg.lib()
    r23 = pkg.CONFIG_CODES["r23_m4"]
    shapes = {
        "k2": pkg.Code(r23["gen1"], 4, 2, 3),
        "n1": pkg.Code([[[1, 1, 1]]], 2, 1, 1),
        "n4": pkg.Code([[[1, 1, 1]], [[1, 0, 1]], [[1, 1, 0]], [[0, 1, 1]]], 2, 1, 4),
        "m9": pkg.Code([[[1] * 10], [[1, 0, 1, 1, 1, 0, 0, 0, 1, 1]]], 9, 1, 2),
    }
    for name, code in shapes.items():
        assert call(pkg, code=code) == -2, name
        assert lib.cvd_last_error().startswith(NAME + b":")
        assert call(pkg, code=code, F=0) == -2, name
    assert call(pkg, code=pkg.Code([[[1, 1]], [[0, 1]]], 1, 1, 2), F=0) == 0
    assert call(pkg, code=pkg.Code([[[1] * 9]] * 3, 8, 1, 3), F=0) == 0


def test_workspace_bytes(pkg, monkeypatch):
    monkeypatch.delenv("CVD_LIST_WAVES", raising=False)
    monkeypatch.delenv("CVD_LIST_LDS_BYTES", raising=False)
    lib = pkg.lib()
    ws, ls = lib.cvd_viterbi_tailbiting_list_workspace_bytes, lib.cvd_viterbi_list_workspace_bytes
    Ts = (1, 16, 17, 64, 65, 100, 1024, 1025, 8192)
    Fs = (1, 2, 63, 1000, 8192, 8193, 1 << 20, I64_MAX)
    for n in (2, 3):
        for m in (1, 2, 6, 7, 8):
            for L in range(1, 9):
                LL = 2 if L <= 2 else 4 if L <= 4 else 8
                step = (1 << m) * LL // 2                     # bytes of a step's decisions
                for T in Ts:
                    ts = min(T, 16384 // step)
                    tile = (ts * step + 15) // 16 * 16
                    slice_ = ((T + ts - 1) // ts - 1) * tile
                    row = [ws(n, m, T, F, L) for F in Fs]
                    assert row == [ls(n, m, T, F, L) for F in Fs]             # the list call's tiling
                    assert all(0 <= s <= GIB and s % 16 == 0 for s in row)
                    if T * step <= 16384:                     # the frame's decisions fit the tile in LDS
                        assert not any(row), (n, m, L, T)
                    else:                                     # a slice per wave, not per frame
                        assert row[0] == slice_ and row[1] == 2 * slice_, (n, m, L, T)
                        assert all(s == min(8192, GIB // slice_) * slice_ for s in row[5:]), (n, m, L, T)
                assert ws(n, m, 100, 0, L) == ws(n, m, 8192, 0, L) == 0
    assert ws(3, 8, 8192, 1, 8) == 511 * 16384
    assert ws(2, 6, 64, 5, 8) == 0 and ws(2, 6, 65, 5, 8) == 5 * 16384 and ws(2, 6, 129, 5, 8) == 5 * 2 * 16384
    assert ws(2, 6, 128, 5, 4) == 0 and ws(2, 6, 129, 5, 3) == 5 * 16384
    for bad in ((1, 6, 100, 5, 4), (4, 6, 100, 5, 4), (2, 0, 100, 5, 4), (2, 9, 100, 5, 4), (2, 6, 0, 5, 4),
                (2, 6, -1, 5, 4), (2, 6, 8193, 5, 4), (2, 6, 100, -1, 4), (2, 6, 100, 5, 0), (2, 6, 100, 5, 9),
                (2, 6, 100, 0, 9)):
        assert ws(*bad) < 0, bad
        assert lib.cvd_last_error().startswith(NAME + b":")
    monkeypatch.setenv("CVD_LIST_WAVES", "3")              # the tests' and the measurement's hooks
    assert ws(2, 6, 65, 10, 8) == 3 * 16384 and ws(2, 6, 65, 2, 8) == 2 * 16384 and ws(2, 6, 64, 10, 8) == 0
    monkeypatch.setenv("CVD_LIST_LDS_BYTES", "4096")
    assert ws(2, 6, 16, 10, 8) == 0 and ws(2, 6, 17, 10, 8) == 3 * 4096
    monkeypatch.setenv("CVD_LIST_LDS_BYTES", "1")          # clamped to 1 KiB: one step of 256 states at L = 8
    assert ws(2, 8, 3, 10, 8) == 3 * 2 * 1024
    monkeypatch.setenv("CVD_LIST_LDS_BYTES", str(1 << 30))  # clamped to 48 KiB
    assert ws(2, 6, 192, 10, 8) == 0 and ws(2, 6, 193, 10, 8) == 3 * 49152


def test_abi_and_exports(pkg):
    assert pkg.lib().cvd_version() == 11
    src = open(os.path.join(ROOT, "include", "cvd.h")).read()
    assert int(re.search(r"#define CVD_ABI_VERSION\s+(\d+)", src).group(1)) == 11
    for name in ("cvd_viterbi_tailbiting_list_workspace_bytes", "cvd_viterbi_decode_frames_tailbiting_list"):
        assert name in pkg._lib.EXPORTS, name
        assert re.search(r"\b" + name + r"\(", src), name
        assert getattr(pkg.lib(), name)
    for name in ("decode_frames_tailbiting_list", "decode_frames_tailbiting_crc"):
        assert callable(getattr(pkg, name)), name
    dec = importlib.import_module(pkg.__name__ + ".decode")
    assert dec.TAILBITING_LAPS == TB.DEFAULT_LAPS and dec.TAILBITING_MAX_LAPS == TB.MAX_LAPS
    mk = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "Makefile")).read()
    assert "cvd_decode_tblist.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^cvd_decode_tblist\.o:", mk, re.M)


def test_wrappers_refuse_bad_arguments(pkg):
    """Every check here comes before the library or the device is asked for anything."""
    cpu = importlib.import_module("torch").device("cpu")
    cap = np.zeros(1000, dtype=np.int8)
    for kw in (dict(T=0), dict(T=8193), dict(T=100, F=6), dict(T=100, start=-1), dict(T=100, stride=0),
               dict(T=100, L=0), dict(T=100, L=9), dict(T=100, max_laps=0), dict(T=100, max_laps=9),
               dict(T=100, max_laps=-1), dict(T=100, offsets=np.zeros(3)), dict(T=100, offsets=np.zeros(3, dtype=np.int32)),
               dict(T=100, offsets=np.zeros(3, dtype=np.int64), F=4), dict(T=100, offsets=[0, 200])):
        kw.setdefault("L", 4)
        with pytest.raises((ValueError, TypeError)):
            pkg.decode_frames_tailbiting_list(2, 6, M6, cap, device=cpu, **kw)
    with pytest.raises(TypeError):
        pkg.decode_frames_tailbiting_list(2, 6, M6, cap.astype(np.uint8), 100, 4, device=cpu)     # hard bits: soft_from_bits first
    with pytest.raises(TypeError):
        pkg.decode_frames_tailbiting_list(2, 6, M6, cap, 100, 4, start_state=0, device=cpu)
    for kw in (dict(crc="crc16"), dict(crc="crc16-ccitt", count=85), dict(crc="crc16-ccitt", first=-1),
               dict(crc="crc16-ccitt", count=-1), dict(crc="crc16-ccitt", first=80, count=5),
               dict(crc="crc16-ccitt", expect=0x10000), dict(crc="crc16-ccitt", expect=-1), dict(crc="crc32", first=69)):
        with pytest.raises(ValueError):
            pkg.decode_frames_tailbiting_crc(2, 6, M6, cap, 100, 4, device=cpu, **kw)

"""cvd_viterbi_decode_frames_llr (max-log-MAP values per bit of framed soft captures) without a
GPU: the reference decoder of llr_cases.py satisfies the identities that include/cvd.h states
(one distance at every step, the saturated set, the bound on finite values, agreement with a
Viterbi traceback wherever L != 0); the exports and the unchanged ABI version; every
invalid-argument case returning CVD_E_INVALID with the entry's name before the device is touched
(the pointers here are never dereferenced); the unsupported shapes; F == 0; the workspace size;
the Python wrapper's and the decode subcommand's argument checks."""
import importlib
import os
import re

import numpy as np
import pytest

import llr_cases as LC
from conftest import ROOT

I64_MAX = (1 << 63) - 1
GIB = 1 << 30
M6 = LC.gen_of(6, 2)
NAME = b"viterbi_decode_frames_llr"

# a valid call of (133,171): five frames of 100 steps from value 3, the last one ending at nvals.
# It is only ever sent with F = 0 or with one argument spoilt: nothing here launches.
GOOD = dict(cap=0x10000, nvals=3 + 5 * 200, start=3, stride=200, offsets=None, F=5, T=100, s0=0, e=0,
            llr=0x70000, bits=0x20000, frames=0x50000, stats=0x30000, work=0x40000)


def call(pkg, code=None, **kw):
    a = dict(GOOD, **kw)
    code = pkg.Code(M6, 6, 1, 2) if code is None else code
    return pkg.lib().cvd_viterbi_decode_frames_llr(code.c, a["cap"], a["nvals"], a["start"], a["stride"], a["offsets"],
                                                   a["F"], a["T"], a["s0"], a["e"], a["llr"], a["bits"], a["frames"],
                                                   a["stats"], a["work"], None)


# ── the contract's identities on the reference ──

IDENTITY_CODES = [(1, 2), (2, 2), (6, 2), (6, 3), (8, 3)]      # (3,1), (7,5), (133,171), (133,171,165), (557,663,711)
BOUNDARIES = [(0, 0), (None, None), (1, None), (None, 1), (1, 1)]


@pytest.mark.parametrize("m,n", IDENTITY_CODES)
def test_reference_satisfies_the_contract(m, n):
    gen = LC.gen_of(m, n)
    S = 1 << m
    rng = np.random.default_rng(1000 * m + n)
    for kind in ("noisy", "m128", "pm1", "zero"):
        for s0, e in BOUNDARIES:
            s0 = None if s0 is None else s0 * (S - 1)         # the nonzero state: all ones
            e = None if e is None else e * (S - 1)
            for T in (m, m + 9, 40) if m < 8 else (m, 21):
                v, _ = LC.soft_frame(rng, gen, n, m, T, s0, e, kind)
                r = LC.reference_frame(gen, n, m, v, T, s0, e)
                dist, u, sT = LC.viterbi_frame(gen, n, m, v, T, s0, e)
                L = r["llr"]
                # one distance at every step, and it is the Viterbi distance
                assert (np.minimum(r["M0"], r["M1"]) == dist).all()
                assert r["record"][0] == dist and r["record"][2] == sT
                # saturated: exactly t >= T - m when the end is fixed, with the tail's sign
                sat = np.abs(L) == LC.SAT
                want = np.arange(T) >= T - m if e is not None else np.zeros(T, dtype=bool)
                assert np.array_equal(sat, want), (kind, s0, e, T)
                if e is not None:
                    for t in range(max(T - m, 0), T):
                        assert L[t] == (LC.SAT if (e >> (T - 1 - t)) & 1 else -LC.SAT)
                # every finite value is bounded
                assert (np.abs(L[~sat]) <= 127 * n * (m + 1)).all()
                # the bits are the traceback's wherever the value decides
                dec = L != 0
                assert np.array_equal(r["bits"][dec], u[dec]), (kind, s0, e, T)
                assert r["record"][1] == int((~dec).sum()) and r["record"][5] == int(sat.sum())
                assert r["record"][4] == (int(np.abs(L[~sat]).min()) if (~sat).any() else LC.SAT)
                if kind == "zero":
                    assert (L[~sat] == 0).all() and r["record"][1] == int((~sat).sum())


def test_minus_128_reads_as_minus_127():
    gen, rng = LC.gen_of(2, 2), np.random.default_rng(5)
    v, _ = LC.soft_frame(rng, gen, 2, 2, 30, 0, 0, "m128")
    assert (v == -128).any()
    w = np.where(v == -128, -127, v).astype(np.int8)
    a, b = LC.reference_frame(gen, 2, 2, v, 30), LC.reference_frame(gen, 2, 2, w, 30)
    assert np.array_equal(a["llr"], b["llr"]) and a["record"] == b["record"]


# ── the library's argument checks ──

INVALID = {
    "T_zero": dict(T=0),
    "T_negative": dict(T=-1),
    "T_above_max": dict(T=65537, nvals=I64_MAX, stride=1 << 20),
    "T_below_m_with_both_states": dict(T=5),
    "start_state_at_2_m": dict(s0=64),
    "start_state_below_any": dict(s0=-2),
    "end_state_at_2_m": dict(e=64),
    "end_state_below_any": dict(e=-2),
    "F_negative": dict(F=-1),
    "F_times_w_is_2_31": dict(T=32, F=1 << 31, stride=1, nvals=I64_MAX),
    "F_times_w_above_2_31": dict(T=33, F=1 << 30, stride=1, nvals=I64_MAX),
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
    "null_llr": dict(llr=None),
    "null_bits": dict(bits=None),
    "null_frames": dict(frames=None),
    "null_stats": dict(stats=None),
    "null_work_where_one_is_needed": dict(work=None),
    "misaligned_capture": dict(cap=0x10008),
    "misaligned_llr_by_8": dict(llr=0x70008),
    "misaligned_llr_by_2": dict(llr=0x70002),
    "misaligned_work": dict(work=0x40008),
    "misaligned_bits": dict(bits=0x20002),
    "misaligned_frames": dict(frames=0x50002),
    "misaligned_stats": dict(stats=0x30004),
    "misaligned_offsets": dict(offsets=0x60004),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments(pkg, case):
    assert call(pkg, F=0) == 0             # the base arguments themselves are valid
    rc = call(pkg, **INVALID[case])
    assert rc == -1, (case, rc)
    msg = pkg.lib().cvd_last_error()
    assert msg and msg.startswith(NAME + b":"), (case, msg)


def test_no_frames_is_ok_without_a_launch(pkg):
    null = dict(cap=None, llr=None, bits=None, frames=None, stats=None, work=None)
    for s0, e in ((0, 0), (-1, -1), (63, -1), (-1, 63)):
        assert call(pkg, F=0, s0=s0, e=e, **null) == 0
    assert call(pkg, F=0, nvals=0, start=0, **null) == 0
    assert call(pkg, F=0, T=0, **null) == 0              # T is a property of the frames
    assert call(pkg, F=0, offsets=0x60000, start=-5, stride=0, **null) == 0      # offset mode ignores both


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
    monkeypatch.delenv("CVD_LLR_WAVES", raising=False)
    lib = pkg.lib()
    ws = lib.cvd_viterbi_llr_workspace_bytes
    Ts = (1, 31, 32, 33, 64, 65, 100, 1024, 1025, 2048, 40000, 65536)
    Fs = (1, 2, 63, 1000, 8192, 8193, 1 << 16, 1 << 20, 1 << 30, I64_MAX)
    for n in (2, 3):
        for m in (1, 2, 6, 7, 8):
            table = [[ws(n, m, T, F) for F in Fs] for T in Ts]
            for T, row in zip(Ts, table):
                slice_ = max((T + 31) // 32 - 2, 0) * (4 << m)     # 2^m int32 per segment but the first and the last
                slice_ = (slice_ + 15) // 16 * 16
                assert all(0 <= s <= GIB for s in row)
                assert all(a <= b for a, b in zip(row, row[1:])), (n, m, row)       # monotone in F
                if T <= 64:                               # one or two segments: no checkpoints
                    assert not any(row), (n, m, T)
                else:                                     # a slice per wave, not per frame
                    assert row[0] == slice_ and row[1] == 2 * slice_, (n, m, T)
                    assert all(s == min(8192, GIB // slice_) * slice_ for s in row[5:]), (n, m, T)
            for col in zip(*table):                       # grows with T at fixed F, until the 1 GiB cap cuts the waves
                assert all(a <= b or b > GIB - (2 << 20) for a, b in zip(col, col[1:])), (n, m, col)
            assert all(s % 16 == 0 for row in table for s in row)
            assert ws(n, m, 100, 0) == ws(n, m, 65536, 0) == 0
    assert ws(2, 6, 64, 5) == 0 and ws(2, 6, 65, 5) == 5 * 256 and ws(2, 6, 128, 5) == 5 * 2 * 256
    assert ws(3, 8, 65536, 1 << 20) == 512 * 2046 * 1024
    for bad in ((1, 6, 100, 5), (4, 6, 100, 5), (2, 0, 100, 5), (2, 9, 100, 5), (2, 6, 0, 5), (2, 6, -1, 5),
                (2, 6, 65537, 5), (2, 6, 100, -1)):
        assert ws(*bad) < 0, bad
        assert lib.cvd_last_error().startswith(NAME + b":")
    monkeypatch.setenv("CVD_LLR_WAVES", "3")               # the tests' and the measurement's hook
    assert ws(2, 6, 128, 10) == 3 * 2 * 256 and ws(2, 6, 128, 2) == 2 * 2 * 256 and ws(2, 6, 64, 10) == 0


def test_abi_and_exports(pkg):
    assert pkg.lib().cvd_version() == 11
    src = open(os.path.join(ROOT, "include", "cvd.h")).read()
    assert int(re.search(r"#define CVD_ABI_VERSION\s+(\d+)", src).group(1)) == 11
    for name in ("cvd_viterbi_llr_workspace_bytes", "cvd_viterbi_decode_frames_llr"):
        assert name in pkg._lib.EXPORTS, name
        assert re.search(r"\b" + name + r"\(", src), name
        assert getattr(pkg.lib(), name)
    assert "CVD_LLR_WAVES" in src
    dec = importlib.import_module(pkg.__name__ + ".decode")
    assert dec.LLR_SATURATED == LC.SAT == 32767
    assert callable(pkg.decode_frames_llr)
    mk = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "Makefile")).read()
    assert "cvd_decode_llr.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1).split()


def test_wrapper_refuses_bad_arguments(pkg):
    """Every check here comes before the library or the device is asked for anything."""
    cpu = importlib.import_module("torch").device("cpu")
    cap = np.zeros(1000, dtype=np.int8)
    for kw in (dict(T=0), dict(T=65537), dict(T=100, F=6), dict(T=100, start=-1), dict(T=100, stride=0),
               dict(T=5), dict(T=100, start_state=64), dict(T=100, end_state=-1),
               dict(T=100, offsets=np.zeros(3)), dict(T=100, offsets=np.zeros(3, dtype=np.int32)),
               dict(T=100, offsets=np.zeros(3, dtype=np.int64), F=4), dict(T=100, offsets=[0, 200])):
        with pytest.raises((ValueError, TypeError)):
            pkg.decode_frames_llr(2, 6, M6, cap, device=cpu, **kw)
    with pytest.raises(TypeError):
        pkg.decode_frames_llr(2, 6, M6, cap.astype(np.uint8), 100, device=cpu)      # hard bits: soft_from_bits first
    with pytest.raises(TypeError):
        pkg.decode_frames_llr(2, 6, M6, cap, 100, keep="dvb:3/4")


def test_parse_decode_llr(pkg):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    base = ["decode", "--code", "oct:133,171", "--input", "cap.npy"]
    assert cli.parse_args(base).llr is False
    a = cli.parse_args(base + ["--frame", "40", "--format", "soft", "--llr"])
    assert (a.frame, a.format, a.llr, a.out_llr, a.start_state, a.end_state) == (40, "soft", True, None, 0, 0)
    a = cli.parse_args(base + ["--frame", "40", "--format", "soft", "--llr", "--end-state", "any", "--out-llr", "x.npy",
                               "--frame-offsets", "off.npy"])
    assert (a.llr, a.end_state, a.out_llr, a.frame_offsets) == (True, None, "x.npy", "off.npy")
    for bad in (["--llr"],                                                   # needs --frame
                ["--llr", "--format", "soft"],
                ["--frame", "40", "--llr"],                                  # needs --format soft
                ["--frame", "40", "--format", "lsb", "--llr"],
                ["--frame", "40", "--format", "soft", "--llr", "--tail-biting"],
                ["--frame", "40", "--format", "soft", "--llr", "--puncture", "dvb:3/4"],
                ["--frame", "40", "--llr", "--puncture", "dvb:3/4"],
                ["--frame", "40", "--format", "soft", "--out-llr", "x.npy"]):   # --out-llr needs --llr
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert cli.LLR_COLUMNS == ["frame", "offset", "status", "distance", "zeros", "weakest", "saturated", "end_state"]
    assert cli.FRAME_COLUMNS == ["frame", "offset", "status", "distance", "errors", "counted", "start_state", "end_state"]

"""cvd_viterbi_decode_frames_list and cvd_frames_crc without a GPU: the reference decoders of
list_cases.py satisfy the consequences that include/cvd.h states (path 0 is the Viterbi path, the
prefix property, ordered distances, distinct rows, the number of paths, the L smallest costs over
all inputs); the CRC reference agrees with the standard library; the exports and the Python copies
of the constants; every invalid-argument case of both entries returning CVD_E_INVALID with the
entry's name before the device is touched (the pointers here are never dereferenced); the
unsupported shapes; F == 0 and rows == 0; the workspace size; crc_spec; the Python wrappers' and
the decode subcommand's argument checks."""
import binascii
import importlib
import os
import re
import zlib

import numpy as np
import pytest

import list_cases as LS
import llr_cases as LC
from conftest import ROOT

I64_MAX = (1 << 63) - 1
GIB = 1 << 30
M6 = LC.gen_of(6, 2)
NAME = b"viterbi_decode_frames_list"
CRC_NAME = b"frames_crc"

# a valid call of (133,171): five frames of 100 steps from value 3, the last one ending at nvals.
# It is only ever sent with F = 0 or with one argument spoilt: nothing here launches.
GOOD = dict(cap=0x10000, nvals=3 + 5 * 200, start=3, stride=200, offsets=None, F=5, T=100, s0=0, e=0, L=4,
            bits=0x20000, paths=0x70000, frames=0x50000, stats=0x30000, work=0x40000)


def call(pkg, code=None, **kw):
    a = dict(GOOD, **kw)
    code = pkg.Code(M6, 6, 1, 2) if code is None else code
    return pkg.lib().cvd_viterbi_decode_frames_list(code.c, a["cap"], a["nvals"], a["start"], a["stride"], a["offsets"],
                                                    a["F"], a["T"], a["s0"], a["e"], a["L"], a["bits"], a["paths"],
                                                    a["frames"], a["stats"], a["work"], None)


# ── the contract's consequences on the reference ──

CONSEQUENCE_CODES = [(1, 2), (2, 2), (3, 2), (6, 2), (6, 3)]     # (3,1), (7,5), (15,17), (133,171), (133,171,165)
BOUNDARIES = [(0, 0), (None, None), (1, None), (None, 1), (1, 1)]


def path_cost(out, cost, m, s0, u):
    """(the cost of the inputs u from state s0, the state after them); out, cost: the code's branch
    outputs and the frame's step costs."""
    s, c = s0, 0
    for t in range(len(u)):
        c += int(cost[t][out[s, int(u[t])]])
        s = ((s << 1) | int(u[t])) & ((1 << m) - 1)
    return c, s


@pytest.mark.parametrize("m,n", CONSEQUENCE_CODES)
def test_reference_satisfies_the_contract(m, n):
    gen = LC.gen_of(m, n)
    S = 1 << m
    rng = np.random.default_rng(1000 * m + n)
    for kind in ("noisy", "pm1", "zero"):
        for s0, e in BOUNDARIES:
            s0 = None if s0 is None else s0 * (S - 1)         # the nonzero state: all ones
            e = None if e is None else e * (S - 1)
            for T in sorted({1, m, m + 1, m + 2, m + 3, 9, 33}):
                if s0 is not None and e is not None and T < m:
                    continue
                v, _ = LC.soft_frame(rng, gen, n, m, T, s0, e, kind)
                out, cost = LC.branch_outputs(gen, n, m), LC.step_costs(v, n, T)
                full = LS.list_frame(gen, n, m, v, T, 8, s0, e)
                if T <= 9:                                    # the two ways of writing the text down agree
                    plain = LS.list_frame_plain(gen, n, m, v, T, 8, s0, e)
                    assert [(p[0], p[1].tolist(), p[2], p[3]) for p in plain] == \
                        [(p[0], p[1].tolist(), p[2], p[3]) for p in full]
                # path 0 is the Viterbi path
                dist, u, sT = LC.viterbi_frame(gen, n, m, v, T, s0, e)
                assert full[0][0] == dist and np.array_equal(full[0][1], u) and full[0][3] == sT
                # every path is a path: its s_0, its bits and the values give its distance and its s_T
                for d, u, a, b in full:
                    assert path_cost(out, cost, m, a, u) == (d, b)
                    assert s0 is None or a == s0
                    assert e is None or b == e
                dists = [p[0] for p in full]
                assert dists == sorted(dists)
                keys = [(p[2] if s0 is None else 0, p[1].tobytes()) for p in full]
                assert len(set(keys)) == len(keys), (kind, s0, e, T)
                if s0 is not None and e is not None:
                    assert len(full) == min(8, 1 << (T - m))
                # the result for L is the first L paths of the result for 8
                for L in (1, 2, 3, 5):
                    part = LS.list_frame(gen, n, m, v, T, L, s0, e)
                    assert len(part) == min(L, len(full))
                    for p, q in zip(part, full):
                        assert p[0] == q[0] and np.array_equal(p[1], q[1]) and p[2:] == q[2:]
                # the L smallest costs over all inputs
                if T <= 9 and s0 is not None:
                    costs = []
                    for x in range(1 << T):
                        u = [(x >> t) & 1 for t in range(T)]
                        c, b = path_cost(out, cost, m, s0, u)
                        if e is None or b == e:
                            costs.append(c)
                    assert dists == sorted(costs)[:8], (kind, s0, e, T)


def test_minus_128_reads_as_minus_127():
    gen, rng = LC.gen_of(2, 2), np.random.default_rng(5)
    v, _ = LC.soft_frame(rng, gen, 2, 2, 30, 0, 0, "m128")
    assert (v == -128).any()
    w = np.where(v == -128, -127, v).astype(np.int8)
    a, b = LS.list_frame(gen, 2, 2, v, 30, 4), LS.list_frame(gen, 2, 2, w, 30, 4)
    assert [(p[0], p[1].tolist()) for p in a] == [(p[0], p[1].tolist()) for p in b]


def test_reference_batch_records():
    gen, rng = LC.gen_of(3, 2), np.random.default_rng(9)
    T, L = 5, 8
    soft = np.concatenate([LC.soft_frame(rng, gen, 2, 3, T, 0, 0)[0] for _ in range(2)])
    bits, paths, frames, stats = LS.reference_batch(gen, 2, 3, soft, T, L, [0, -1, 10, 11], 0, 0)
    assert bits.shape == (4, L, 4) and paths.shape == (4, L, 3) and frames.tolist() == [[4, 0], [0, 1], [4, 0], [0, 1]]
    assert (paths[0, 4:] == -1).all() and not bits[0, 4:].any() and (paths[1] == -1).all() and not bits[1].any()
    assert stats == [int(paths[0, 0, 0] + paths[2, 0, 0]), 2, 2, 8, 1]


# ── the CRC reference against the standard library ──

def test_crc_reference_against_the_standard_library():
    rng = np.random.default_rng(3)
    for nbytes in (1, 2, 7, 33):
        data = rng.integers(0, 256, nbytes, dtype=np.uint8)
        msb = np.unpackbits(data, bitorder="big")
        assert LS.crc_bits(msb, 16, 0x1021, 0) == binascii.crc_hqx(data.tobytes(), 0)
        # CRC-32 as Ethernet and 802.11 send it: the bytes LSB first, init all ones, the FCS complemented
        lsb = np.unpackbits(data, bitorder="little")
        reg = LS.crc_bits(lsb, 32, 0x04C11DB7, 0xFFFFFFFF)
        z = zlib.crc32(data.tobytes())
        assert int(f"{reg:032b}"[::-1], 2) ^ 0xFFFFFFFF == z
        fcs = np.unpackbits(np.frombuffer(z.to_bytes(4, "little"), dtype=np.uint8), bitorder="little")
        u = np.concatenate([lsb, fcs])
        assert LS.crc_value(u, 0, 8 * nbytes, 32, 0x04C11DB7, 0xFFFFFFFF) == 0xFFFFFFFF
        u[3] ^= 1
        assert LS.crc_value(u, 0, 8 * nbytes, 32, 0x04C11DB7, 0xFFFFFFFF) != 0xFFFFFFFF
        # an appended CRC-16 gives 0; masked with an RNTI it gives the RNTI
        assert LS.crc_value(LS.crc_append(msb, 16, 0x1021), 0, 8 * nbytes, 16, 0x1021) == 0
        assert LS.crc_value(LS.crc_append(msb, 16, 0x1021, 0, 0xBEEF), 0, 8 * nbytes, 16, 0x1021) == 0xBEEF
        # first and count: bits before and behind do not enter
        pad = np.concatenate([[1, 0, 1], LS.crc_append(msb, 24, 0x864CFB), [1, 1]]).astype(np.uint8)
        assert LS.crc_value(pad, 3, 8 * nbytes, 24, 0x864CFB) == 0
    rows = rng.integers(0, 256, (2, 3, 8), dtype=np.uint8)
    vals = LS.reference_crc(rows, 1, 40, 8, 0x9B, 0)
    assert vals.shape == (2, 3) and vals[1, 2] == LS.crc_value(LS.unpack_rows(rows)[1, 2], 1, 40, 8, 0x9B)
    present = np.array([[True, True, True], [True, True, False]])
    assert LS.select(np.array([[5, 0, 0], [1, 2, 0]]), present, 0).tolist() == [1, -1]


# ── the library's argument checks ──

INVALID = {
    "T_zero": dict(T=0),
    "T_negative": dict(T=-1),
    "T_above_max": dict(T=8193, nvals=I64_MAX, stride=1 << 20),
    "T_below_m_with_both_states": dict(T=5),
    "L_zero": dict(L=0),
    "L_negative": dict(L=-1),
    "L_above_max": dict(L=9),
    "start_state_at_2_m": dict(s0=64),
    "start_state_below_any": dict(s0=-2),
    "end_state_at_2_m": dict(e=64),
    "end_state_below_any": dict(e=-2),
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
    for s0, e in ((0, 0), (-1, -1), (63, -1), (-1, 63)):
        for L in (1, 8):
            assert call(pkg, F=0, s0=s0, e=e, L=L, **null) == 0
    assert call(pkg, F=0, nvals=0, start=0, **null) == 0
    assert call(pkg, F=0, T=0, **null) == 0              # T is a property of the frames
    assert call(pkg, F=0, T=8193, **null) == 0
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
    monkeypatch.delenv("CVD_LIST_WAVES", raising=False)
    monkeypatch.delenv("CVD_LIST_LDS_BYTES", raising=False)
    lib = pkg.lib()
    ws = lib.cvd_viterbi_list_workspace_bytes
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
                    assert all(0 <= s <= GIB and s % 16 == 0 for s in row)
                    assert all(a <= b for a, b in zip(row, row[1:])), (n, m, L, T, row)       # monotone in F
                    if T * step <= 16384:                     # the frame's decisions fit the tile in LDS
                        assert not any(row), (n, m, L, T)
                    else:                                     # a slice per wave, not per frame
                        assert row[0] == slice_ and row[1] == 2 * slice_, (n, m, L, T)
                        assert all(s == min(8192, GIB // slice_) * slice_ for s in row[5:]), (n, m, L, T)
                assert ws(n, m, 100, 0, L) == ws(n, m, 8192, 0, L) == 0
    assert ws(2, 1, 1, 1, 1) == 0 and ws(2, 1, 8192, 1 << 20, 2) == 0          # the smallest shape; two states never leave LDS
    assert ws(3, 8, 8192, 1, 8) == 511 * 16384                                  # the largest: 8 MiB per wave but a tile
    assert ws(3, 8, 8192, 1 << 20, 8) == (GIB // (511 * 16384)) * 511 * 16384
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


CRC_GOOD = dict(bits=0x20000, rows=7, w=4, first=3, count=80, width=16, poly=0x1021, init=0, value=0x80000)
CRC_INVALID = {
    "width_zero": dict(width=0, poly=0),
    "width_negative": dict(width=-1, poly=0),
    "width_33": dict(width=33),
    "poly_at_2_width": dict(poly=0x10000),
    "poly_above_width_8": dict(width=8, poly=0x19B),
    "init_at_2_width": dict(init=0x10000),
    "first_negative": dict(first=-1),
    "count_negative": dict(count=-1),
    "field_one_past_the_row": dict(first=32, count=81),
    "count_overflows_int32_sums": dict(first=(1 << 31) - 1, count=(1 << 31) - 1),
    "w_zero": dict(w=0, first=0, count=0, width=1, poly=1),
    "w_negative": dict(w=-1),
    "rows_negative": dict(rows=-1),
    "null_bits": dict(bits=None),
    "null_value": dict(value=None),
    "misaligned_bits": dict(bits=0x20002),
    "misaligned_value": dict(value=0x80001),
}


def crc_call(pkg, **kw):
    a = dict(CRC_GOOD, **kw)
    return pkg.lib().cvd_frames_crc(a["bits"], a["rows"], a["w"], a["first"], a["count"], a["width"], a["poly"], a["init"],
                                    a["value"], None)


@pytest.mark.parametrize("case", sorted(CRC_INVALID))
def test_crc_invalid_arguments(pkg, case):
    assert crc_call(pkg, rows=0) == 0      # the base arguments themselves are valid
    rc = crc_call(pkg, **CRC_INVALID[case])
    assert rc == -1, (case, rc)
    msg = pkg.lib().cvd_last_error()
    assert msg and msg.startswith(CRC_NAME + b":"), (case, msg)


def test_crc_no_rows_is_ok_without_a_launch(pkg):
    assert crc_call(pkg, rows=0, bits=None, value=None) == 0
    assert crc_call(pkg, rows=0, bits=0x20002, value=0x80001) == 0
    assert crc_call(pkg, rows=0, first=32, count=80) == 0            # the field ends exactly at 32 w
    assert crc_call(pkg, rows=0, width=32, poly=0xFFFFFFFF, init=0xFFFFFFFF, count=0, first=96) == 0
    assert crc_call(pkg, rows=0, width=1, poly=1, init=1) == 0
    assert crc_call(pkg, rows=0, first=32, count=81) == -1           # the arguments are still checked


def test_abi_and_exports(pkg):
    assert pkg.lib().cvd_version() == 11
    src = open(os.path.join(ROOT, "include", "cvd.h")).read()
    for name in ("cvd_viterbi_list_workspace_bytes", "cvd_viterbi_decode_frames_list", "cvd_frames_crc"):
        assert name in pkg._lib.EXPORTS, name
        assert re.search(r"\b" + name + r"\(", src), name
        assert getattr(pkg.lib(), name)
    assert int(re.search(r"#define CVD_VITERBI_LIST_MAX_L\s+(\d+)", src).group(1)) == 8
    assert int(re.search(r"#define CVD_VITERBI_LIST_MAX_T\s+(\d+)", src).group(1)) == 8192
    assert "CVD_LIST_WAVES" in src and "CVD_LIST_LDS_BYTES" in src
    dec = importlib.import_module(pkg.__name__ + ".decode")
    assert dec.LIST_MAX_L == LS.MAX_L == 8 and dec.LIST_MAX_T == LS.MAX_T == 8192
    assert dec.CRC_SPECS == LS.CRC_SPECS == pkg.CRC_SPECS
    for name in ("decode_frames_list", "decode_frames_crc", "frames_crc", "crc_spec"):
        assert callable(getattr(pkg, name)), name
    mk = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "Makefile")).read()
    assert "cvd_decode_list.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1).split()


def test_crc_spec(pkg):
    assert pkg.crc_spec("crc8-lte") == (8, 0x9B, 0, 0)
    assert pkg.crc_spec("crc16-ccitt") == (16, 0x1021, 0, 0)
    assert pkg.crc_spec("crc24a") == (24, 0x864CFB, 0, 0)
    assert pkg.crc_spec("crc24b") == (24, 0x800063, 0, 0)
    assert pkg.crc_spec("crc32") == (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF)
    assert pkg.crc_spec("16:1021") == (16, 0x1021, 0, 0)
    assert pkg.crc_spec("16:8005:ffff") == (16, 0x8005, 0xFFFF, 0)
    assert pkg.crc_spec("32:04C11DB7:FFFFFFFF:ffffffff") == pkg.crc_spec("crc32")
    assert pkg.crc_spec("1:1") == (1, 1, 0, 0)
    assert pkg.crc_spec((5, 0x15, 0x1F, 0)) == (5, 0x15, 0x1F, 0)
    for bad in ("crc16", "", "16", "16:", "0:1", "33:1", "16:10000", "16:1021:10000", "16:1021:0:10000", "16:1021:0:0:0",
                "x:1", "16:g", "-1:1", (16, 0x1021), (16, 0x1021, 0, -1)):
        with pytest.raises(ValueError):
            pkg.crc_spec(bad)


def test_wrappers_refuse_bad_arguments(pkg):
    """Every check here comes before the library or the device is asked for anything."""
    cpu = importlib.import_module("torch").device("cpu")
    cap = np.zeros(1000, dtype=np.int8)
    for kw in (dict(T=0), dict(T=8193), dict(T=100, F=6), dict(T=100, start=-1), dict(T=100, stride=0), dict(T=5),
               dict(T=100, L=0), dict(T=100, L=9), dict(T=100, start_state=64), dict(T=100, end_state=-1),
               dict(T=100, offsets=np.zeros(3)), dict(T=100, offsets=np.zeros(3, dtype=np.int32)),
               dict(T=100, offsets=np.zeros(3, dtype=np.int64), F=4), dict(T=100, offsets=[0, 200])):
        kw.setdefault("L", 4)
        with pytest.raises((ValueError, TypeError)):
            pkg.decode_frames_list(2, 6, M6, cap, device=cpu, **kw)
    with pytest.raises(TypeError):
        pkg.decode_frames_list(2, 6, M6, cap.astype(np.uint8), 100, 4, device=cpu)     # hard bits: soft_from_bits first
    for kw in (dict(crc="crc16"), dict(crc="crc16-ccitt", count=79), dict(crc="crc16-ccitt", first=-1),
               dict(crc="crc16-ccitt", count=-1), dict(crc="crc16-ccitt", first=80, count=5),
               dict(crc="crc16-ccitt", expect=0x10000), dict(crc="crc16-ccitt", expect=-1),
               dict(crc="crc32", end_state=None, first=69)):
        with pytest.raises(ValueError):
            pkg.decode_frames_crc(2, 6, M6, cap, 100, 4, device=cpu, **kw)
    rows = np.zeros((3, 8), dtype=np.uint8)
    for bits, first, count, spec in ((rows, 0, 49, "crc16-ccitt"), (rows, -1, 8, "crc16-ccitt"), (rows, 0, -1, "crc8-lte"),
                                     (rows, 0, 8, "crc9"), (rows, 60, 0, "crc8-lte")):
        with pytest.raises(ValueError):
            pkg.frames_crc(bits, first, count, spec, device=cpu)
    for bits in (rows.astype(np.int8), np.zeros((3, 7), dtype=np.uint8), np.zeros((3, 0), dtype=np.uint8),
                 np.uint8(3), [[0, 0, 0, 0]]):
        with pytest.raises(TypeError):
            pkg.frames_crc(bits, 0, 8, "crc8-lte", device=cpu)


def test_parse_decode_list(pkg):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    base = ["decode", "--code", "oct:133,171", "--input", "cap.npy"]
    a = cli.parse_args(base)
    assert (a.list, a.crc, a.crc_first, a.crc_count, a.crc_expect) == (None, None, None, None, None)
    a = cli.parse_args(base + ["--frame", "40", "--format", "soft", "--list", "4"])
    assert (a.frame, a.format, a.list, a.crc, a.start_state, a.end_state) == (40, "soft", 4, None, 0, 0)
    a = cli.parse_args(base + ["--frame", "122", "--format", "soft", "--list", "8", "--crc", "crc16-ccitt", "--crc-first",
                               "2", "--crc-count", "98", "--crc-expect", "beef", "--end-state", "any", "--frame-offsets",
                               "off.npy"])
    assert (a.list, a.crc, a.crc_first, a.crc_count, a.crc_expect, a.end_state) == (8, "crc16-ccitt", 2, 98, 0xBEEF, None)
    assert cli.parse_args(base + ["--frame", "40", "--format", "soft", "--list", "2", "--crc", "16:8005:ffff"]).crc == \
        "16:8005:ffff"
    ok = ["--frame", "40", "--format", "soft", "--list", "4"]
    for bad in (["--list", "4"],                                             # needs --frame
                ["--list", "4", "--format", "soft"],
                ["--frame", "40", "--list", "4"],                            # needs --format soft
                ["--frame", "40", "--format", "lsb", "--list", "4"],
                ok + ["--tail-biting"],
                ok + ["--puncture", "dvb:3/4"],
                ok + ["--llr"],
                ok + ["--T", "100"],
                ok + ["--sync", "100"],
                ["--format", "soft", "--list", "4", "--T", "100"],
                ["--frame", "40", "--format", "soft", "--list", "0"],
                ["--frame", "40", "--format", "soft", "--list", "9"],
                ok + ["--crc", "crc16"],                                     # an unknown CRC
                ok + ["--crc-first", "2"],                                   # --crc* need --crc
                ok + ["--crc-count", "20"],
                ok + ["--crc-expect", "0"],
                ["--frame", "40", "--format", "soft", "--crc", "crc16-ccitt"],      # --crc needs --list
                ["--frame", "40", "--format", "soft", "--crc-first", "2"],
                ["--crc", "crc16-ccitt"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    assert cli.LIST_COLUMNS == ["frame", "path", "offset", "status", "distance", "start_state", "end_state"]
    assert cli.CRC_COLUMNS == ["frame", "offset", "status", "paths", "choice", "crc_ok", "distance", "distance0",
                               "start_state", "end_state"]
    assert cli.FRAME_COLUMNS == ["frame", "offset", "status", "distance", "errors", "counted", "start_state", "end_state"]

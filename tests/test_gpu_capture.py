"""Captured bitstreams on the GPU: cvd_pack_windows against a numpy restatement of the
header's semantics (whole buffer, zero padding included), a round trip with the generator,
and Detector.scan / the scan subcommand against the C oracle's per-trial sums, bit for bit.
Every expected value is an exact reference value; no test asserts a statistical outcome.
The shapes are the smallest at which the kernel can still go wrong (tile edges at 64
sequences and 32 chunks, ragged last words, n = 3's 30-bit words), not the workload's."""
import csv
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import parity as OP
from test_gpu_parity import pack_words, unpack_words

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


# ───────────────────────────── numpy restatement ────────────────────────────

def raw_capture(bits, fmt, rng):
    """uint8 buffer of a capture holding `bits`, padded to 16 bytes; every bit and byte of
    the buffer past the capture's last bit is ones (they must never reach the output).
    BYTES format: bit b = byte[b] & 1, the bytes' upper bits are noise."""
    nbits = len(bits)
    if fmt == "bytes":
        raw = np.full((nbits + 15) // 16 * 16, 0xFF, np.uint8)
        raw[:nbits] = bits | (rng.integers(0, 128, nbits).astype(np.uint8) << 1)
        return raw
    padded = np.ones((nbits + 127) // 128 * 128, np.uint8)
    padded[:nbits] = bits
    return np.packbits(padded, bitorder="little" if fmt == "lsb" else "big")


def capture_bits(raw, fmt, nbits):
    """include/cvd.h CVD_CAPTURE_*: bit b of the capture."""
    if fmt == "bytes":
        return raw[:nbits] & 1
    return np.unpackbits(raw, bitorder="little" if fmt == "lsb" else "big")[:nbits]


def pack_restatement(bits, n, N, start, stride, nwin, n_phase, pitch=None, q0=0, fill=0):
    """cvd_pack_windows, as include/cvd.h states it: uint32 [W4/4, pitch, 4]."""
    spw = 32 // n
    W = (N + spw - 1) // spw
    W4 = (W + 3) // 4 * 4
    nseq = nwin * n_phase
    pitch = q0 + nseq if pitch is None else pitch
    q = np.arange(nseq, dtype=np.int64)
    first = start + (q // n_phase) * stride + q % n_phase            # window i, phase f
    assert nseq == 0 or first[-1] + N * n <= len(bits)
    wb = np.zeros((nseq, W4 * spw * n), np.uint64)
    wb[:, :N * n] = bits[first[:, None] + np.arange(N * n, dtype=np.int64)[None, :]]
    # word w = steps [w*spw, +spw): step t's output j at bit n*(t % spw) + j
    words = (wb.reshape(nseq, W4, spw * n) << np.arange(spw * n, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    out = np.full((W4 // 4, pitch, 4), fill, np.uint32)
    out[:, q0:q0 + nseq, :] = words.reshape(nseq, W4 // 4, 4).transpose(1, 0, 2)
    return out


PACK_CASES = [
    # n, N, start, stride, nwin, n_phase, format
    (2, 37, 0, 74, 130, 1, "bytes"),
    (2, 64, 5, 128, 65, 2, "lsb"),        # exactly four words; unaligned start
    (2, 1001, 13, 77, 300, 2, "msb"),     # overlapping; odd stride
    (1, 129, 3, 129, 70, 1, "lsb"),
    (3, 23, 1, 69, 67, 3, "bytes"),
    (3, 1001, 31, 3003, 130, 3, "msb"),
    (2, 1, 0, 2, 200, 1, "lsb"),
    # more than one tile of 32 chunks along a window (tile = block)
    (2, 8197, 7, 16397, 70, 2, "bytes"),  # 129 chunks: five tiles, the last of one chunk
    (3, 1327, 2, 1000, 66, 2, "lsb"),     # 34 chunks of 120 bits; overlapping
    (1, 16641, 1, 501, 65, 1, "msb"),     # 131 chunks; heavily overlapping
]


def _pack_case(pkg, case, q0=0, extra_pitch=0):
    n, N, start, stride, nwin, n_phase, fmt = case
    rng = np.random.default_rng(hash(case[:6]) & 0xFFFF)
    nbits = start + (nwin - 1) * stride + (n_phase - 1) + N * n    # the last window ends on the last bit
    assert nbits % 32 != 0
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    raw = raw_capture(bits, fmt, rng)
    assert np.array_equal(capture_bits(raw, fmt, nbits), bits)
    det = pkg.Detector(1, n, 2, [[[1, 1, 1]]] * n, device=0)
    nseq = nwin * n_phase
    pitch = q0 + nseq + extra_pitch
    out = torch.full((det.words_per_seq(N) // 4, pitch, 4), SENTINEL, dtype=torch.int32, device="cuda")
    buf, got_nwin = det.pack_capture(torch.from_numpy(raw).cuda(), N, start=start, stride=stride, n_phase=n_phase,
                                     format=fmt, nbits=nbits, out=out, q0=q0, pitch=pitch)
    assert got_nwin == nwin and buf is out
    want = pack_restatement(bits, n, N, start, stride, nwin, n_phase, pitch, q0, fill=SENTINEL)
    assert torch.equal(buf.cpu(), torch.from_numpy(want.view(np.int32)))


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: "n{}_N{}_s{}_d{}_w{}_f{}_{}".format(*c))
def test_pack_equals_restatement(pkg, case):
    _pack_case(pkg, case)


def test_pack_q0_pitch_leaves_other_columns(pkg):
    """q0 = 3 and pitch = nseq + 9 into a sentinel-filled buffer: columns outside
    [q0, q0 + nseq) keep the sentinel."""
    _pack_case(pkg, PACK_CASES[2], q0=3, extra_pitch=6)


def test_pack_host_array_defaults(pkg):
    """A host numpy capture (uploaded, padded), nbits / stride / nwin defaults: as many whole
    windows as fit, the tail bits unused."""
    n, N = 2, 50
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, 100 * 7 + 37).astype(np.uint8)
    det = pkg.Detector(1, n, 2, [[[1, 1, 1]]] * n, device=0)
    buf, nwin = det.pack_capture(bits, N)
    assert nwin == 7
    assert torch.equal(buf.cpu(), torch.from_numpy(pack_restatement(bits, n, N, 0, N * n, 7, 1).view(np.int32)))
    packed = np.packbits(bits)                       # MSB first: numpy's default
    buf, nwin = det.pack_capture(packed, N, format="msb", nbits=len(bits), n_phase=2)
    assert nwin == 7
    assert torch.equal(buf.cpu(), torch.from_numpy(pack_restatement(bits, n, N, 0, N * n, 7, 2).view(np.int32)))


# ─────────────────────────── round trip with the generator ──────────────────

def serial_bits(words, n):
    """received words [N, nseq] -> serial bits [nseq, N*n] (bit n*t + j = output j of step t)."""
    w = np.asarray(words, np.int64).T
    return ((w[:, :, None] >> np.arange(n)) & 1).reshape(w.shape[0], -1).astype(np.uint8)


def test_generate_unpack_pack_round_trip(pkg):
    cc = pkg.CONFIG_CODES["m6"]
    det = pkg.Detector(1, 2, 6, cc["gen1"], device=0)
    N, count = 517, 130
    gen = det.generate(cc["gen1"], N, 0.05, 99, 17, 0, 1, count)
    words = unpack_words(gen, 2, N)
    capture = serial_bits(words, 2).reshape(-1)
    buf, nwin = det.pack_capture(np.packbits(capture), N, format="msb", nbits=len(capture))
    assert nwin == count
    np.testing.assert_array_equal(unpack_words(buf, 2, N), words)


# ───────────────────────── scan against the C oracle ─────────────────────────

JUNK = 13   # bits before the first window
SCAN = {
    "m2": dict(code="m2", learn_len=None, N=200, p=0.05, trials=12),
    "m6": dict(code="m6", learn_len=30_000, N=400, p=0.05, trials=8),   # sparse model, bit-sliced kernel
}
SEED = 12345


@pytest.fixture(scope="module")
def oracle_capture(pkg):
    """Per configuration: the oracle's trial streams H1_0, H2_0, H1_1, ... (sequence ids 2t
    and 2t + 1, oracle/cvd_oracle.c:379-380) as one capture behind 13 junk bits (3 more after
    the last window), the oracle's per-trial sums, and the detector and model."""
    out = {}
    rng = np.random.default_rng(11)
    for name, cfg in SCAN.items():
        cc = pkg.CONFIG_CODES[cfg["code"]]
        m, N, p, T = cc["m"], cfg["N"], cfg["p"], cfg["trials"]
        c1, c2 = C.Code(cc["gen1"], m, 1, 2), C.Code(cc["gen2"], m, 1, 2)
        tag = C.lib().oc_grid_tag(N, p)
        streams = [C.stream(c1 if sid % 2 == 0 else c2, N, p, SEED, tag, sid) for sid in range(2 * T)]
        bits = np.concatenate([rng.integers(0, 2, JUNK).astype(np.uint8),
                               serial_bits(np.stack(streams, axis=1), 2).reshape(-1),
                               rng.integers(0, 2, 3).astype(np.uint8)])
        _, sums = C.Model(c1, p, cfg["learn_len"], 200, 1.0, SEED).run_trials(c1, c2, N, p, SEED, 0, T, sums=True)
        det = pkg.Detector(1, 2, m, cc["gen1"], device=0)
        model = det.model(p, cfg["learn_len"], 200, 1.0, SEED)
        out[name] = dict(cfg, cc=cc, streams=streams, bits=bits, sums=sums.reshape(2 * T, 2), det=det, model=model)
    return out


@pytest.mark.parametrize("name", ["m2", "m6"])
def test_scan_sums_equal_oracle(pkg, oracle_capture, name):
    o = oracle_capture[name]
    inf = o["model"].info()
    assert inf["kind"] == (0 if name == "m2" else 1)
    if name == "m6" and os.environ.get("CVD_BITSLICE", "1") != "0":
        assert inf["explicit_kernel"] == 5, inf   # the bit-sliced kernel
    res = o["det"].scan(o["model"], o["bits"], o["N"], start=JUNK)
    nwin = 2 * o["trials"]
    assert res["logp1"].shape == res["logref"].shape == res["h1"].shape == (nwin, 1)
    assert np.array_equal(res["offset"][:, 0], JUNK + np.arange(nwin) * o["N"] * 2)
    assert np.array_equal(res["logp1"][:, 0], o["sums"][:, 0])
    assert np.array_equal(res["logref"][:, 0], o["sums"][:, 1])
    assert np.array_equal(res["llr"], res["logp1"] - res["logref"])
    assert np.array_equal(res["h1"][:, 0], o["sums"][:, 0] > o["sums"][:, 1])
    assert np.array_equal(res["best_phase"], np.zeros(nwin, np.int64))
    # the same capture packed LSB- and MSB-first
    for fmt in ("lsb", "msb"):
        packed = np.packbits(o["bits"], bitorder="little" if fmt == "lsb" else "big")
        r2 = o["det"].scan(o["model"], packed, o["N"], start=JUNK, format=fmt, nbits=len(o["bits"]))
        assert np.array_equal(r2["logp1"], res["logp1"]) and np.array_equal(r2["logref"], res["logref"])


def test_scan_phases(pkg, oracle_capture):
    o = oracle_capture["m2"]
    det, N = o["det"], o["N"]
    nwin = 2 * o["trials"]
    res = det.scan(o["model"], o["bits"], N, start=JUNK, n_phase=2)
    assert res["logp1"].shape == (nwin, 2)
    assert np.array_equal(res["logp1"][:, 0], o["sums"][:, 0]) and np.array_equal(res["logref"][:, 0], o["sums"][:, 1])
    # phase 1: the windows one bit later, packed on the host
    shifted = [o["bits"][JUNK + 1 + i * 2 * N:JUNK + 1 + (i + 1) * 2 * N].reshape(N, 2) for i in range(nwin)]
    r = pack_words([s[:, 0] | (s[:, 1] << 1) for s in shifted], 2)
    sums = torch.full((nwin, 2), float("nan"), dtype=torch.float64, device="cuda")
    det.detect(o["model"], r, N, nwin, nwin, sums=sums)
    sums = sums.cpu().numpy()
    assert np.array_equal(res["logp1"][:, 1], sums[:, 0]) and np.array_equal(res["logref"][:, 1], sums[:, 1])
    assert np.array_equal(res["offset"][:, 1], res["offset"][:, 0] + 1)
    assert np.array_equal(res["best_phase"], np.argmax(res["llr"], axis=1))


def test_scan_batching(pkg, oracle_capture):
    """batch = 7 windows (four launches, the last of 3) equals the single batch exactly."""
    o = oracle_capture["m2"]
    for n_phase in (1, 2):
        one = o["det"].scan(o["model"], o["bits"], o["N"], start=JUNK, n_phase=n_phase)
        cut = o["det"].scan(o["model"], o["bits"], o["N"], start=JUNK, n_phase=n_phase, batch=7)
        assert sorted(one) == sorted(cut)
        for key in one:
            assert np.array_equal(one[key], cut[key]), (n_phase, key)
        assert np.array_equal(cut["logp1"][:, 0], o["sums"][:, 0])
        assert np.array_equal(cut["logref"][:, 0], o["sums"][:, 1])


@pytest.mark.parametrize("name", ["m2", "m6"])
def test_scan_parity_column(pkg, oracle_capture, name):
    o = oracle_capture[name]
    tpl = pkg.default_template(o["cc"]["gen1"], o["cc"]["m"])
    res = o["det"].scan(o["model"], o["bits"], o["N"], start=JUNK, parity_template=tpl, batch=5)
    want = [OP.satisfied_count(OP.streams_from_words(s, 2), tpl) for s in o["streams"]]
    assert np.array_equal(res["parity_sat"][:, 0], [w[0] for w in want])
    assert np.array_equal(res["parity_frac"][:, 0], [w[0] / w[1] for w in want])
    assert np.array_equal(res["logp1"][:, 0], o["sums"][:, 0])


def test_scan_capture_one_call(pkg, oracle_capture):
    o = oracle_capture["m2"]
    cc = o["cc"]
    res = pkg.scan_capture(1, 2, cc["m"], cc["gen1"], o["bits"], o["N"], o["p"], start=JUNK)
    assert np.array_equal(res["logp1"][:, 0], o["sums"][:, 0]) and np.array_equal(res["logref"][:, 0], o["sums"][:, 1])


def test_scan_cli(pkg, oracle_capture, tmp_path):
    o = oracle_capture["m2"]
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    npy, out = str(tmp_path / "capture.npy"), str(tmp_path / "scan.csv")
    np.save(npy, o["bits"])
    assert cli.main(["scan", "--code", "m2", "--p", "0.05", "--N", "200", "--input", npy, "--phases", "2",
                     "--out", out]) == 0
    want = o["det"].scan(o["model"], o["bits"], 200, n_phase=2)
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["window", "phase", "offset", "logp1", "logref", "llr", "h1"]
    nwin = want["logp1"].shape[0]
    assert nwin == 2 * o["trials"] and len(rows) == 1 + 2 * nwin
    for i in range(nwin):
        for f in range(2):
            row = rows[1 + 2 * i + f]
            assert [int(row[0]), int(row[1]), int(row[2]), int(row[6])] == \
                [i, f, int(want["offset"][i, f]), int(want["h1"][i, f])]
            # floats are written as repr: they read back exactly
            assert [float(x) for x in row[3:6]] == [want[c][i, f] for c in ("logp1", "logref", "llr")]
            assert row[3:6] == [repr(float(want[c][i, f])) for c in ("logp1", "logref", "llr")]

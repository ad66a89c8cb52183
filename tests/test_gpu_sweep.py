"""Blind parity-check search on the GPU: cvd_parity_sweep against a numpy restatement of the
header's semantics (sliding words -> np.bincount -> int64 Walsh-Hadamard transform ->
(T + w) // 2, the whole [n_phase, 2^B] array), accumulation, agreement with
cvd_parity_detect, and find_parity_checks / identify_code / the identify subcommand against
the ranking rule restated here, on the C oracle's streams.  Every expected value is an exact
reference value; no test asserts a statistical outcome.  The shapes are the smallest at which
the kernels can still go wrong (B = 14..17 and 20..22 around the two regime boundaries, n = 3's
words that are not dword-periodic, a T below a wave, several blocks with a ragged tail)."""
import csv
import ctypes
import importlib
import math
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from test_gpu_capture import JUNK, SCAN, SEED, capture_bits, raw_capture, serial_bits

pytestmark = pytest.mark.gpu


# ───────────────────────────── numpy restatement ────────────────────────────

def wht(v):
    """W[a] = sum_x v[x] (-1)^popcount(a & x), int64."""
    v = np.asarray(v, np.int64).copy()
    h = 1
    while h < len(v):
        p = v.reshape(-1, 2, h)
        v = np.stack([p[:, 0, :] + p[:, 1, :], p[:, 0, :] - p[:, 1, :]], axis=1).reshape(-1)
        h *= 2
    return v


def sweep_restatement(bits, n, span, start, T, n_phase):
    """cvd_parity_sweep into a zeroed d_sat, as include/cvd.h states it: int64 [n_phase, 2^B]."""
    B = n * (span + 1)
    out = np.zeros((n_phase, 1 << B), np.int64)
    for f in range(n_phase):
        first = start + f + n * np.arange(T, dtype=np.int64)
        assert T == 0 or first[-1] + B <= len(bits)
        words = (bits[first[:, None] + np.arange(B)[None, :]].astype(np.int64) << np.arange(B)).sum(axis=1)
        out[f] = (T + wht(np.bincount(words, minlength=1 << B))) // 2
    return out


def ranking_restatement(sat, T, n, top=16, z_min=None):
    """find_parity_checks' rule on a sat array [n, 2^B]."""
    n_phase, size = sat.shape
    if z_min is None:
        z_min = math.sqrt(2.0 * math.log(n_phase * float(size))) + 3.0
    d = 2 * sat - T
    sig = d.astype(np.float64) ** 2 >= z_min * z_min * T
    sig[:, 0] = False
    items = []
    for f, mask in zip(*np.nonzero(sig)):
        f, mask = int(f), int(mask)
        set_bits = [b for b in range(size.bit_length()) if (mask >> b) & 1]
        lo, hi = set_bits[0] // n, set_bits[-1] // n
        extent = hi - lo + 1
        # mask bit n*e + j: output j of symbol e, i.e. delay hi - e of the shortest window
        tpl = sorted((b % n, hi - b // n) for b in set_bits)
        s = int(sat[f, mask])
        items.append(((extent, -abs(2 * s - T), f, mask),
                      {"phase": f, "mask": mask, "extent": extent, "mask0": mask >> (n * lo), "template": tpl,
                       "sat": s, "T": T, "z": (2 * s - T) / math.sqrt(T), "inverted": 2 * s < T}))
    return [e for _, e in sorted(items, key=lambda it: it[0])][:top]


# ─────────────────────── the sweep against the restatement ──────────────────

SWEEP_CASES = [
    # n, span, start, T, n_phase, format
    (1, 3, 3, 1000, 1, "lsb"),
    (2, 0, 0, 1, 1, "bytes"),
    (2, 6, 13, 4001, 2, "msb"),        # B = 14: one below the LDS / global boundary
    (3, 4, 31, 2999, 3, "bytes"),      # B = 15: the last whole histogram in LDS, 136 KiB
    (2, 7, 5, 70001, 2, "lsb"),        # B = 16: the first in parts of 2^15 bins; three tiles, ragged tail
    (3, 5, 2, 5003, 3, "msb"),         # B = 18
    (2, 10, 7, 9001, 1, "lsb"),        # B = 22: global atomics
    (1, 16, 11, 3001, 1, "msb"),       # B = 17
    (2, 9, 3, 6001, 2, "bytes"),       # B = 20
    (3, 6, 4, 4001, 3, "lsb"),         # B = 21: the last in parts (64 of them)
    (2, 3, 1, 37, 2, "msb"),           # T below a wave
    (2, 6, 9, 100003, 2, "bytes"),     # whole-LDS regime over four blocks, ragged tail
    (3, 3, 127, 50021, 3, "lsb"),      # n = 3 across three tiles, first word on a piece's last bit
]


def sweep_nbits(n, span, start, T, n_phase):
    """The last word ends on the capture's last bit."""
    return start + (n_phase - 1) + n * (T - 1) + n * (span + 1)


def raw_sweep(pkg, cap, nbits, fmt, n, span, start, T, n_phase, sat):
    """cvd_parity_sweep itself, accumulating into the int64 device tensor `sat`."""
    L = pkg.lib()
    work = torch.empty(L.cvd_parity_sweep_workspace_bytes(n, span, n_phase), dtype=torch.uint8, device="cuda")
    pkg._lib.check(L.cvd_parity_sweep(ctypes.c_void_p(cap.data_ptr()), nbits, pkg._lib.CAPTURE_FORMATS[fmt], n,
                                      span, start, T, n_phase, ctypes.c_void_p(sat.data_ptr()),
                                      ctypes.c_void_p(work.data_ptr()),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return sat


@pytest.mark.parametrize("case", SWEEP_CASES, ids=lambda c: "n{}_s{}_st{}_T{}_f{}_{}".format(*c))
def test_sweep_equals_restatement(pkg, case):
    n, span, start, T, n_phase, fmt = case
    rng = np.random.default_rng(hash(case[:5]) & 0xFFFF)
    nbits = sweep_nbits(n, span, start, T, n_phase)
    assert nbits % 32 != 0
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    raw = raw_capture(bits, fmt, rng)                      # every bit past nbits is a one
    assert np.array_equal(capture_bits(raw, fmt, nbits), bits)
    got = pkg.parity_sweep(raw, n, span, start=start, T=T, n_phase=n_phase, format=fmt, nbits=nbits)
    assert got.dtype == torch.int64 and tuple(got.shape) == (n_phase, 1 << (n * (span + 1)))
    want = sweep_restatement(bits, n, span, start, T, n_phase)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.all(want[:, 0] == T)
    # T=None: as many anchors as fit, which here is T
    if T < 5000:
        again = pkg.parity_sweep(torch.from_numpy(raw).cuda(), n, span, start=start, n_phase=n_phase, format=fmt,
                                 nbits=nbits)
        assert torch.equal(again, got)


@pytest.mark.parametrize("value", [0, 1])
def test_constant_capture(pkg, value):
    """Every anchor in one bin.  All zeros: every template is satisfied by every anchor;
    all ones: the templates of even weight are, the others never."""
    n, span, start, T, n_phase = 2, 6, 5, 70_001, 2
    nbits = sweep_nbits(n, span, start, T, n_phase)
    bits = np.full(nbits, value, np.uint8)
    got = pkg.parity_sweep(raw_capture(bits, "lsb", None), n, span, start=start, T=T, n_phase=n_phase,
                           format="lsb", nbits=nbits).cpu().numpy()
    if value == 0:
        assert np.all(got == T)
    else:
        weight = np.array([bin(m).count("1") for m in range(1 << 14)])
        assert np.array_equal(got, np.broadcast_to(np.where(weight % 2 == 0, T, 0), got.shape))


@pytest.mark.parametrize("span", [6, 7, 10], ids=["B14_lds", "B16_lds_parts", "B22_global"])
def test_accumulation(pkg, span):
    """d_sat is accumulated, not cleared: two calls on adjacent anchor ranges equal one call
    over both, and a second identical call doubles the array."""
    n, start, T, n_phase = 2, 3, 3001, 2
    rng = np.random.default_rng(21)
    nbits = sweep_nbits(n, span, start, T, n_phase)
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    cap = torch.from_numpy(raw_capture(bits, "msb", rng)).cuda()
    size = 1 << (n * (span + 1))
    one = raw_sweep(pkg, cap, nbits, "msb", n, span, start, T, n_phase,
                    torch.zeros((n_phase, size), dtype=torch.int64, device="cuda"))
    assert np.array_equal(one.cpu().numpy(), sweep_restatement(bits, n, span, start, T, n_phase))
    T0 = 1234
    two = torch.zeros((n_phase, size), dtype=torch.int64, device="cuda")
    raw_sweep(pkg, cap, nbits, "msb", n, span, start, T0, n_phase, two)
    raw_sweep(pkg, cap, nbits, "msb", n, span, start + n * T0, T - T0, n_phase, two)
    assert torch.equal(two, one)
    raw_sweep(pkg, cap, nbits, "msb", n, span, start, T, n_phase, two)
    assert torch.equal(two, 2 * one)


def test_bit_positions_past_2_31_and_split_calls(pkg):
    """A packed capture of 2^31 + 2^20 + 3 bits (256 MiB): words that begin past bit 2^31
    against the restatement on those bytes, and T=None, which is more than 2^31 - 1 anchors:
    parity_sweep splits it into two calls that accumulate.  The single-bit masks of the
    whole sweep are checked against the capture's popcount."""
    n, span = 1, 3
    nbits = (1 << 31) + (1 << 20) + 3
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    cap = torch.randint(0, 256, (((nbits + 7) // 8 + 15) // 16 * 16,), dtype=torch.uint8, device="cuda", generator=gen)
    start, T = (1 << 31) + 12345, 70_001
    tail = np.unpackbits(cap[start // 8:(start + T + span) // 8 + 1].cpu().numpy(), bitorder="little")
    got = pkg.parity_sweep(cap, n, span, start=start, T=T, format="lsb", nbits=nbits)
    assert np.array_equal(got.cpu().numpy(), sweep_restatement(tail, n, span, start % 8, T, 1))
    T_all = nbits - span
    assert T_all > (1 << 31) - 1 and T_all % 8 == 0
    total = pkg.parity_sweep(cap, n, span, format="lsb", nbits=nbits)
    assert int(total[0, 0]) == T_all
    first = (1 << 31) - 1
    parts = torch.zeros_like(total)
    raw_sweep(pkg, cap, nbits, "lsb", n, span, 0, first, 1, parts)
    raw_sweep(pkg, cap, nbits, "lsb", n, span, first, T_all - first, 1, parts)
    assert torch.equal(total, parts)
    # mask 1 << i: the anchors whose bit i is 0, i.e. the zeros among bits [i, i + T_all)
    raw = cap.cpu().numpy()
    ones_per_byte = np.array([bin(v).count("1") for v in range(256)], np.uint8)
    ones = int(ones_per_byte[raw[:T_all // 8]].sum(dtype=np.int64))        # bits [0, T_all)
    bit = lambda b: int(raw[b >> 3] >> (b & 7)) & 1                         # noqa: E731
    for i in range(span + 1):
        assert int(total[0, 1 << i]) == T_all - ones, i
        ones += bit(T_all + i) - bit(i)                                     # -> bits [i + 1, i + 1 + T_all)


# ───────────────────────────── oracle streams ───────────────────────────────

def oracle_bits(pkg, name, which, N, p, junk=JUNK):
    """`junk` random bits, the oracle's stream 0 of the configuration's gen1 / gen2 at grid
    point (N, p) serialised, and 3 more random bits."""
    cc = pkg.CONFIG_CODES[name]
    code = C.Code(cc[which], cc["m"], cc["k"], cc["n"])
    words = C.stream(code, N, p, SEED, C.lib().oc_grid_tag(N, p), 0)
    rng = np.random.default_rng(11)
    return np.concatenate([rng.integers(0, 2, junk).astype(np.uint8),
                           serial_bits(np.stack([words], axis=1), cc["n"]).reshape(-1),
                           rng.integers(0, 2, 3).astype(np.uint8)])


@pytest.mark.parametrize("name", ["m2", "m6"])
def test_agrees_with_parity_detect(pkg, name):
    """sat[f][template_mask] of the sweep = cvd_parity_detect's satisfied count on the same
    bits packed as one window of N = T + span steps from bit start + f."""
    cc = pkg.CONFIG_CODES[name]
    tpl = pkg.default_template(cc["gen1"], cc["m"])
    span = max(s for _, s in tpl)
    T, start = 1000, JUNK
    bits = oracle_bits(pkg, name, "gen1", T + span + 1, 0.05)
    sat = pkg.parity_sweep(bits, 2, span, start=start, T=T, n_phase=2).cpu().numpy()
    det = pkg.Detector(1, 2, cc["m"], cc["gen1"], device=0)
    mask = pkg.template_mask(tpl, 2, span)
    assert pkg.mask_template(mask, 2, span) == sorted(tpl)
    for f in range(2):
        r, nwin = det.pack_capture(bits, T + span, start=start + f, nwin=1)
        d_sat = torch.zeros(1, dtype=torch.int32, device="cuda")
        pkg.parity_detect(r, 2, T + span, 1, 1, tpl, 0.6, sat=d_sat)
        assert int(sat[f, mask]) == int(d_sat.item()), (name, f)


IDENTIFY_CASES = [
    # configuration, generator, N, p, max_span
    ("m6", "gen1", 4000, 0.05, 7), ("m6", "gen2", 4000, 0.05, 7),
    ("m6", "gen1", 4000, 0.05, 8), ("m6", "gen2", 4000, 0.05, 8),
    ("m6", "gen1", 1500, 0.0, 7), ("m6", "gen2", 1500, 0.0, 7),
    ("m2", "gen1", 600, 0.05, 4), ("m2", "gen2", 600, 0.05, 4),
]


@pytest.mark.parametrize("case", IDENTIFY_CASES, ids=lambda c: "{}_{}_N{}_p{}_s{}".format(*c))
def test_identify(pkg, case):
    name, which, N, p, max_span = case
    cc = pkg.CONFIG_CODES[name]
    bits = oracle_bits(pkg, name, which, N, p)
    T = N - max_span
    for start, phase in ((JUNK, 0), (JUNK - 1, 1)):
        want = ranking_restatement(sweep_restatement(bits, 2, max_span, start, T, 2), T, 2)
        got = pkg.find_parity_checks(bits, 2, max_span, start=start, T=T)
        assert got == want
        assert len(got) > 0 and got[0]["template"] == pkg.mask_template(got[0]["mask0"], 2, got[0]["extent"] - 1)
        ident = pkg.identify_code(bits, max_span, start=start, T=T)
        assert ident["gen"] == cc[which] and ident["m"] == cc["m"] and ident["phase"] == phase
        assert ident["check"] == want[0]
    # all of them, and a higher bar
    assert pkg.find_parity_checks(bits, 2, max_span, start=JUNK, T=T, top=None) == \
        ranking_restatement(sweep_restatement(bits, 2, max_span, JUNK, T, 2), T, 2, top=None)
    assert pkg.find_parity_checks(bits, 2, max_span, start=JUNK, T=T, z_min=20.0, top=3) == \
        ranking_restatement(sweep_restatement(bits, 2, max_span, JUNK, T, 2), T, 2, top=3, z_min=20.0)


def test_identify_random_bits_is_none(pkg):
    N, max_span = 4000, 7
    bits = np.random.default_rng(7).integers(0, 2, JUNK + 2 * N + 3).astype(np.uint8)
    T = N - max_span
    assert ranking_restatement(sweep_restatement(bits, 2, max_span, JUNK, T, 2), T, 2) == []
    assert pkg.find_parity_checks(bits, 2, max_span, start=JUNK, T=T) == []
    assert pkg.identify_code(bits, max_span, start=JUNK, T=T) is None


def test_rate_two_thirds_ranking(pkg):
    """r23_m4 (k = 2, n = 3): the ranked list equals the restatement; its phase is not a
    claim (a one-bit shift can keep a check's extent there)."""
    N, p, max_span = 3000, 0.02, 5
    bits = oracle_bits(pkg, "r23_m4", "gen1", N, p)
    T = N - max_span
    want = ranking_restatement(sweep_restatement(bits, 3, max_span, JUNK, T, 3), T, 3)
    got = pkg.find_parity_checks(bits, 3, max_span, start=JUNK, T=T)
    assert got == want and len(got) > 0
    # packed MSB-first: the same list
    packed = np.packbits(bits)
    assert pkg.find_parity_checks(packed, 3, max_span, start=JUNK, T=T, format="msb", nbits=len(bits)) == want


# ─────────────────────────────── command line ───────────────────────────────

def test_identify_cli(pkg, tmp_path, capsys):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    cc = pkg.CONFIG_CODES["m6"]
    bits = oracle_bits(pkg, "m6", "gen1", 4000, 0.05)
    npy, out = str(tmp_path / "capture.npy"), str(tmp_path / "identify.csv")
    np.save(npy, bits)
    assert cli.main(["identify", "--input", npy, "--n", "2", "--max-span", "7", "--start", str(JUNK),
                     "--out", out]) == 0
    want = pkg.find_parity_checks(bits, 2, 7, start=JUNK)
    with open(out, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["rank", "phase", "mask", "extent", "sat", "T", "z", "equation"]
    assert len(want) > 0 and len(rows) == 1 + len(want)
    for rank, (row, c) in enumerate(zip(rows[1:], want)):
        assert [int(row[0]), int(row[1]), int(row[2], 16), int(row[3]), int(row[4]), int(row[5]), float(row[6])] == \
            [rank, c["phase"], c["mask"], c["extent"], c["sat"], c["T"], c["z"]]
        h = [[int((j, s) in c["template"]) for s in range(c["extent"])] for j in range(2)]
        assert row[7] == pkg.parity_vector_to_equation(h)
    printed = capsys.readouterr().out
    code = re.search(r"--code (oct:[0-7,]+)", printed).group(1)
    assert code == "oct:133,171"
    assert cli.code_of(code) == (1, 2, 6, cc["gen1"], cc["gen2"])
    assert f"--start {JUNK} " in printed


def test_scan_cli_octal_code(pkg, tmp_path):
    """scan --code oct:133,171 is scan --code m6: the same CSV, to the last digit."""
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    cfg, cc = SCAN["m6"], pkg.CONFIG_CODES["m6"]
    N, p, trials = cfg["N"], cfg["p"], 4
    c1, c2 = C.Code(cc["gen1"], 6, 1, 2), C.Code(cc["gen2"], 6, 1, 2)
    tag = C.lib().oc_grid_tag(N, p)
    streams = [C.stream(c1 if sid % 2 == 0 else c2, N, p, SEED, tag, sid) for sid in range(2 * trials)]
    rng = np.random.default_rng(11)
    bits = np.concatenate([rng.integers(0, 2, JUNK).astype(np.uint8),
                           serial_bits(np.stack(streams, axis=1), 2).reshape(-1)])
    npy = str(tmp_path / "capture.npy")
    np.save(npy, bits)
    text = {}
    for code in ("m6", "oct:133,171"):
        out = str(tmp_path / (code.replace(":", "_").replace(",", "_") + ".csv"))
        assert cli.main(["scan", "--code", code, "--p", str(p), "--N", str(N), "--input", npy, "--start", str(JUNK),
                         "--learn-len", str(cfg["learn_len"]), "--out", out]) == 0
        text[code] = open(out).read()
    assert text["m6"] == text["oct:133,171"]
    assert len(text["m6"].splitlines()) == 1 + 2 * trials

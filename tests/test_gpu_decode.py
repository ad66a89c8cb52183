"""Hard-decision Viterbi decoding of a capture on the GPU: cvd_viterbi_decode against a numpy
restatement of the header's sequential decoder (vectorised over the states) and of its counter
definitions (warm vectors, lookahead certification), on the C oracle's streams behind a junk
prefix.  Every expected value is exact; no test asserts a statistical outcome.  The shapes are
the smallest at which the kernels can still go wrong: 2^m below, at and above a wavefront's 64
lanes, n = 3's symbols that are not dword-periodic, T of one step, below a word, below a block,
a whole number of blocks, a ragged tail, more than twenty blocks, and T below the warm-up."""
import csv
import importlib
import re

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from test_gpu_capture import JUNK, SEED, capture_bits, raw_capture, serial_bits

pytestmark = pytest.mark.gpu

POP = np.array([bin(v).count("1") for v in range(8)], np.int64)

CODES = {
    # name: (octal spec, capture format of its cases)
    "m2": ("oct:7,5", "bytes"),              # 4 states: fewer than a wave's lanes
    "m3n3": ("oct:13,15,17", "msb"),         # n = 3: symbols not dword-periodic
    "m6": ("oct:133,171", "lsb"),            # exactly 64 states
    "m8": ("oct:561,753", "msb"),            # 256 states: four per lane
}
TMAX = 4817                                  # 150 blocks of 32 and 17 steps


# ───────────────────────────── numpy restatement ────────────────────────────

class Trellis:
    """States and branches of include/cvd.h: bit 0 of a state is the most recent input."""

    def __init__(self, gen, n, m):
        self.n, self.m, self.S = n, m, 1 << m
        s = np.arange(self.S)
        self.out = np.zeros((self.S, 2), np.int64)               # out[s, u]
        for j in range(n):
            taps = list(gen[j][0]) + [0] * (m + 1 - len(gen[j][0]))
            reg = np.zeros(self.S, np.int64)
            for d in range(1, m + 1):
                reg ^= taps[d] * ((s >> (d - 1)) & 1)
            for u in range(2):
                self.out[:, u] |= ((taps[0] * u) ^ reg) << j
        sp = np.arange(self.S)                                   # next state s'
        self.u = sp & 1
        self.ps = [(sp >> 1) | (b << (m - 1)) for b in range(2)]
        self.o = [self.out[self.ps[b], self.u] for b in range(2)]

    def step(self, D, y):
        """One Eq. 4-5 step on D [..., S] with received words y [...]: (D', decisions)."""
        y = np.asarray(y)[..., None]
        c0 = D[..., self.ps[0]] + POP[self.o[0] ^ y]
        c1 = D[..., self.ps[1]] + POP[self.o[1] ^ y]
        dec = c1 < c0                                            # ties keep b = 0
        Dn = np.where(dec, c1, c0)
        return Dn - Dn.min(axis=-1, keepdims=True), dec


def symbols(bits, n, start, T):
    """y_t: capture bit start + n*t + j is output j of step t."""
    return (bits[start:start + n * T].reshape(T, n).astype(np.int64) << np.arange(n)).sum(axis=1)


def forward(tr, y):
    """D_0 .. D_T [T+1, S] and dec_0 .. dec_{T-1} [T, S] of the sequential recursion."""
    T = len(y)
    Dall = np.zeros((T + 1, tr.S), np.int64)
    dec = np.zeros((T, tr.S), np.int64)
    for t in range(T):
        Dall[t + 1], dec[t] = tr.step(Dall[t], y[t])
    assert Dall.max() <= tr.n * tr.m
    return Dall, dec


def traceback(tr, y, Dall, dec, T):
    """bits, errors, s_0, s_T of the first T steps."""
    sT = int(np.argmax(Dall[T] == 0))                            # the lowest-index state with D_T = 0
    s, errors = sT, 0
    bits = np.zeros(T, np.uint8)
    for t in range(T - 1, -1, -1):
        u = s & 1
        prev = (s >> 1) | (int(dec[t, s]) << (tr.m - 1))
        bits[t] = u
        errors += int(POP[tr.out[prev, u] ^ y[t]])
        s = prev
    return bits, errors, s, sT


def counters(tr, y, Dall, dec, T, L, W, Dp):
    """(blocks, forward reruns, traceback fix-ups) as include/cvd.h defines them."""
    nb = (T + L - 1) // L
    b = np.arange(1, nb)
    reruns = 0
    if len(b):
        # the warm vectors of all blocks at once: block b steps through t = bL - W + j
        Dw = np.zeros((len(b), tr.S), np.int64)
        for j in range(W):
            t = b * L - W + j
            live = t >= 0
            if not live.any():
                continue
            Dn, _ = tr.step(Dw, y[np.maximum(t, 0)])
            Dw = np.where(live[:, None], Dn, Dw)
        reruns = int((Dw != Dall[b * L]).any(axis=1).sum())
    bb = np.arange(nb)
    e = np.minimum(T, (bb + 1) * L + Dp)
    look = bb[e < T]                                             # the others trace from the true s_T
    fixups = 0
    if len(look):
        s = np.broadcast_to(np.arange(tr.S), (len(look), tr.S)).copy()
        for j in range(Dp):                                      # e_b = (b+1)L + Dp for all of them
            t = (look + 1) * L + Dp - 1 - j
            s = (s >> 1) | (dec[t[:, None], s] << (tr.m - 1))
        fixups = int((s != s[:, :1]).any(axis=1).sum())
    return nb, reruns, fixups


def restatement(tr, bits, start, T, L, W, Dp, fwd=None):
    y = symbols(bits, tr.n, start, T)
    Dall, dec = fwd if fwd is not None else forward(tr, y)
    ub, errors, s0, sT = traceback(tr, y, Dall, dec, T)
    nb, reruns, fixups = counters(tr, y, Dall, dec, T, L, W, Dp)
    return {"bits": ub, "T": T, "errors": errors, "ber": errors / (tr.n * T), "start_state": s0, "end_state": sT,
            "blocks": nb, "forward_reruns": reruns, "trace_fixups": fixups, "block": L, "warm": W, "depth": Dp}


def unpacked(res):
    """The decoded bits of a decode_capture result; the bits of the last word past T are zero."""
    raw = res["bits"].cpu().numpy()
    assert raw.dtype == np.uint8 and raw.size == (res["T"] + 31) // 32 * 4
    allb = np.unpackbits(raw, bitorder="little")
    assert not allb[res["T"]:].any()
    return allb[:res["T"]]


def check(res, want):
    assert np.array_equal(unpacked(res), want["bits"])
    got = {k: v for k, v in res.items() if k != "bits"}
    assert got == {k: v for k, v in want.items() if k != "bits"}


# ───────────────────────────── oracle streams ───────────────────────────────

_CACHE = {}


def code_of(pkg, name):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    k, n, m, gen, _ = cli.code_of(CODES[name][0])
    assert k == 1
    return n, m, gen


def oracle_case(pkg, name, p):
    """(trellis, gen, capture bits, forward pass of the TMAX steps from bit JUNK): JUNK random
    bits, the oracle's stream 0 of the code at (TMAX, p) serialised, 3 more random bits.  Built
    once per (code, p) and not changed."""
    key = (name, p)
    if key not in _CACHE:
        n, m, gen = code_of(pkg, name)
        words = C.stream(C.Code(gen, m, 1, n), TMAX, p, SEED, C.lib().oc_grid_tag(TMAX, p), 0)
        rng = np.random.default_rng(11)
        bits = np.concatenate([rng.integers(0, 2, JUNK).astype(np.uint8),
                               serial_bits(np.stack([words], axis=1), n).reshape(-1),
                               rng.integers(0, 2, 3).astype(np.uint8)])
        tr = Trellis(gen, n, m)
        fwd = forward(tr, symbols(bits, n, JUNK, TMAX))
        for a in fwd:
            a.setflags(write=False)
        _CACHE[key] = (tr, gen, bits, fwd)
    return _CACHE[key]


SHAPES = [
    # T, block, warm, depth
    (1, 32, 64, 40),
    (31, 32, 64, 40),
    (200, 256, 64, 40),            # T < L: a single block
    (768, 256, 64, 40),            # T = 3L exactly
    (1297, 256, 100, 40),          # T = 5L + 17: a ragged tail, e_b clipped at T
    (4817, 32, 64, 40),            # 151 blocks; warm-up and lookahead span several blocks
    (50, 32, 100, 40),             # T < W
    (1100, 1056, 64, 8),           # L not a multiple of 64 (a 32-step last chunk), segments of 1,024 steps
]


@pytest.mark.parametrize("p", [0.0, 0.05])
@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_equals_restatement(pkg, name, p):
    tr, gen, bits, fwd = oracle_case(pkg, name, p)
    fmt = CODES[name][1]
    assert JUNK % 8 != 0
    rng = np.random.default_rng(3)
    raw = raw_capture(bits, fmt, rng)                    # every bit past the capture is a one
    assert np.array_equal(capture_bits(raw, fmt, len(bits)), bits)
    cap = torch.from_numpy(raw).cuda()
    for T, L, W, Dp in SHAPES:
        want = restatement(tr, bits, JUNK, T, L, W, Dp, fwd=(fwd[0][:T + 1], fwd[1][:T]))
        res = pkg.decode_capture(tr.n, tr.m, gen, cap, start=JUNK, T=T, format=fmt, nbits=len(bits), block=L,
                                 warm=W, depth=Dp)
        check(res, want)
    # the other two formats, and T=None: as many whole symbols as fit (the 3 tail bits: one more for n = 2, 3)
    T_all = (len(bits) - JUNK) // tr.n
    want = restatement(tr, bits, JUNK, T_all, 256, 64, 40)
    for other in sorted({"bytes", "lsb", "msb"} - {fmt}):
        res = pkg.decode_capture(tr.n, tr.m, gen, raw_capture(bits, other, rng), start=JUNK, format=other,
                                 nbits=len(bits), block=256, warm=64, depth=40)
        check(res, want)


def test_both_fallback_paths_run_and_stay_exact(pkg):
    """warm = 0, depth = 0: every join and every lookahead that the restatement says fails must
    be counted, and the result must equal the generous call's, where none fails."""
    tr, gen, bits, fwd = oracle_case(pkg, "m6", 0.05)
    T, L = TMAX, 32
    none = restatement(tr, bits, JUNK, T, L, 0, 0, fwd=fwd)
    assert none["forward_reruns"] > 0 and none["trace_fixups"] > 0
    res0 = pkg.decode_capture(2, 6, gen, bits, start=JUNK, T=T, block=L, warm=0, depth=0)
    check(res0, none)
    generous = restatement(tr, bits, JUNK, T, L, 1536, 512, fwd=fwd)
    assert generous["forward_reruns"] == 0 and generous["trace_fixups"] == 0
    res1 = pkg.decode_capture(2, 6, gen, bits, start=JUNK, T=T, block=L, warm=1536, depth=512)
    check(res1, generous)
    assert torch.equal(res0["bits"], res1["bits"]) and res0["errors"] == res1["errors"]
    # in between: some joins and some lookaheads fail, not all
    some = restatement(tr, bits, JUNK, T, L, 24, 12, fwd=fwd)
    assert 0 < some["forward_reruns"] < some["blocks"] - 1 and 0 < some["trace_fixups"] < some["blocks"] - 1
    check(pkg.decode_capture(2, 6, gen, bits, start=JUNK, T=T, block=L, warm=24, depth=12), some)


def test_block_split_independence(pkg):
    tr, gen, bits, _ = oracle_case(pkg, "m8", 0.05)
    runs = [pkg.decode_capture(2, 8, gen, bits, start=JUNK, T=TMAX, block=b, warm=w, depth=d)
            for b, w, d in ((32, 0, 0), (256, 300, 100), (None, None, None))]
    assert runs[2]["block"] == 4096 and runs[2]["blocks"] == 2
    for r in runs[1:]:
        assert torch.equal(r["bits"], runs[0]["bits"])
        assert (r["errors"], r["start_state"], r["end_state"]) == \
            (runs[0]["errors"], runs[0]["start_state"], runs[0]["end_state"])


@pytest.mark.parametrize("name", ["m3n3", "m6"])
def test_noiseless_capture_reencodes(pkg, name):
    """p = 0: no channel errors, and encoding the decoded bits from the start state gives the
    capture's symbols back."""
    tr, gen, bits, _ = oracle_case(pkg, name, 0.0)
    res = pkg.decode_capture(tr.n, tr.m, gen, bits, start=JUNK, T=TMAX, block=256)
    assert res["errors"] == 0 and res["ber"] == 0.0
    u = unpacked(res)
    s, y = res["start_state"], np.zeros(TMAX, np.int64)
    for t in range(TMAX):
        y[t] = tr.out[s, u[t]]
        s = ((s << 1) | int(u[t])) & (tr.S - 1)
    assert s == res["end_state"]
    assert np.array_equal(y, symbols(bits, tr.n, JUNK, TMAX))


@pytest.mark.parametrize("value", [0, 1])
@pytest.mark.parametrize("name", ["m2", "m6", "m8"])
def test_constant_capture(pkg, name, value):
    """Tie-heavy: the tie rule, and survivors that do not merge."""
    n, m, gen = code_of(pkg, name)
    tr = Trellis(gen, n, m)
    T, start = 1000, 5
    bits = np.full(start + n * T + 1, value, np.uint8)
    for L, W, Dp in ((32, 64, 40), (256, 0, 0)):
        want = restatement(tr, bits, start, T, L, W, Dp)
        check(pkg.decode_capture(n, m, gen, bits, start=start, T=T, block=L, warm=W, depth=Dp), want)


def test_bit_positions_past_2_31(pkg):
    """A packed random capture of 2^31 + 2^20 bits (256 MiB): symbols that begin past bit 2^31
    against the restatement on those bytes."""
    n, m, gen = code_of(pkg, "m6")
    tr = Trellis(gen, n, m)
    nbits = (1 << 31) + (1 << 20)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    cap = torch.randint(0, 256, (nbits // 8,), dtype=torch.uint8, device="cuda", generator=g)
    start, T = (1 << 31) + 12345, 2001
    tail = np.unpackbits(cap[start // 8:(start + n * T) // 8 + 1].cpu().numpy(), bitorder="little")
    want = restatement(tr, tail, start % 8, T, 256, 64, 40)
    check(pkg.decode_capture(n, m, gen, cap, start=start, T=T, format="lsb", nbits=nbits, block=256, warm=64,
                             depth=40), want)


def test_decoded_bits_are_a_capture(pkg):
    """The decoded bits go back into the existing tools as a format="lsb" capture of T bits."""
    tr, gen, bits, _ = oracle_case(pkg, "m6", 0.05)
    res = pkg.decode_capture(2, 6, gen, bits, start=JUNK, T=TMAX)
    span = 5
    sat = pkg.parity_sweep(res["bits"], 1, span, format="lsb", nbits=res["T"])
    assert int(sat[0][0]) == TMAX - span                 # every anchor satisfies the empty template
    # mask 1: the anchors whose first bit is 0
    assert int(sat[0][1]) == int((unpacked(res)[:TMAX - span] == 0).sum())


def test_decode_cli(pkg, tmp_path, capsys):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    tr, gen, bits, _ = oracle_case(pkg, "m6", 0.05)
    npy, out = str(tmp_path / "capture.npy"), str(tmp_path / "res")
    np.save(npy, bits)
    assert cli.main(["decode", "--code", "oct:133,171", "--input", npy, "--start", str(JUNK), "--save-dir", out]) == 0
    want = pkg.decode_capture(2, 6, gen, bits, start=JUNK)
    got = np.load(str(tmp_path / "res" / "decoded.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, want["bits"].cpu().numpy())
    with open(str(tmp_path / "res" / "decode.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["T", "errors", "ber", "start_state", "end_state", "blocks", "forward_reruns", "trace_fixups"]
    assert len(rows) == 2
    assert [float(v) if c == "ber" else int(v) for c, v in zip(rows[0], rows[1])] == [want[c] for c in rows[0]]
    printed = capsys.readouterr().out
    assert re.search(r"--p (\S+)", printed).group(1) == repr(want["ber"])
    assert want["errors"] > 0
    line = re.search(r"scan --code (\S+) --start (\d+) --input (\S+) --format (\S+) --p \S+ --N N", printed)
    assert line.groups() == ("oct:133,171", str(JUNK), npy, "bytes")

"""cvd_encode_frames without a GPU: the tests' reference encoder (encode_cases.py) reproduces the
reference project's own encoder on the five golden pairs and equals the host encoders the decoder
tests carry; every CVD_E_INVALID / CVD_E_UNSUPPORTED case of the header comes back before the
device is touched, naming encode_frames (the pointers here are never dereferenced); F == 0; the
exports; the shapes of the GPU round trips through the frame, stream and tail-biting decoders are
vetted on the tests' host decoders; the wrappers' and the command line's refusals."""
import importlib
import os
import re

import numpy as np
import pytest

import encode_cases as EC
import llr_cases as LC
import tblist_cases as TB
import test_gpu_decode_frames as TF
import test_gpu_decode_tailbite as TG
from conftest import ROOT

I64_MAX = (1 << 63) - 1
M6 = LC.gen_of(6, 2)
NAME = b"encode_frames"


# ── the reference encoder ──

def test_reference_reproduces_the_golden_pairs():
    pairs = EC.golden_pairs()
    assert len(pairs) == 5
    for name, gen, m, u, v in pairs:
        n, T = len(gen), len(u) + m
        assert v.shape == (n, T) and T == 40 + m
        row = np.concatenate([u, np.ones(m, np.uint8)])           # the tail is forced to 0 whatever the row holds
        got = EC.frame_bits(gen, n, m, row, T, EC.TERMINATED)
        assert np.array_equal(got.reshape(T, n).T, v), name
        buf, written, skipped = EC.encode_ref(gen, n, m, [row], T, EC.TERMINATED)
        assert (written, skipped) == (1, 0) and np.array_equal(buf[:n * T], got) and not buf[n * T:].any()


def test_reference_equals_the_decoder_tests_encoders():
    rng = np.random.default_rng(5)
    for m, n in EC.DECODER_SHAPES:
        gen = EC.gen_of(m, n)
        for T in (1, m - 1, m, m + 1, 33, 70):
            if T < 1:
                continue
            u = rng.integers(0, 2, T).astype(np.uint8)
            for s0 in (0, 1, (1 << m) - 1, int(rng.integers(1 << m))):
                want, _ = LC.encode(gen, n, m, u, s0)
                assert np.array_equal(EC.frame_bits(gen, n, m, u, T, EC.OPEN, s0), want), (m, n, T, s0)
            want, _ = TB.encode_circular(gen, n, m, u)                                   # T < m included
            assert np.array_equal(EC.frame_bits(gen, n, m, u, T, EC.TAILBITING), want), (m, n, T)


def test_reference_formats_and_pattern():
    gen, rng = M6, np.random.default_rng(6)
    u = rng.integers(0, 2, (3, 20)).astype(np.uint8)
    full = [EC.frame_bits(gen, 2, 6, u[f], 20, EC.OPEN, 5) for f in range(3)]
    keep = [3, 2, 1]
    for f in range(3):
        kept = [full[f][2 * t + j] for t in range(20) for j in range(2) if (keep[t % 3] >> j) & 1]
        assert np.array_equal(EC.frame_bits(gen, 2, 6, u[f], 20, EC.OPEN, 5, keep), kept)
    assert EC.span_of(2, 20, keep) == 27
    by, _, _ = EC.encode_ref(gen, 2, 6, u, 20, EC.OPEN, 5, nout=150, start=3, stride=45)
    assert len(by) == 160 and np.array_equal(by[3:43], full[0]) and np.array_equal(by[93:133], full[2])
    assert not by[:3].any() and not by[43:48].any() and not by[133:].any()
    so, _, _ = EC.encode_ref(gen, 2, 6, u, 20, EC.OPEN, 5, format="soft", amplitude=24, nout=150, start=3, stride=45)
    sv = so.view(np.int8)
    assert np.array_equal(sv[3:43], 24 * (2 * full[0].astype(np.int8) - 1)) and not sv[43:48].any()
    msb, _, _ = EC.encode_ref(gen, 2, 6, u, 20, EC.OPEN, 5, format="msb", nout=150, start=3, stride=45)
    assert np.array_equal(msb[:19], np.packbits(by[:150]))
    lsb, _, _ = EC.encode_ref(gen, 2, 6, u, 20, EC.OPEN, 5, format="lsb", nout=150, start=3, stride=45)
    assert np.array_equal(np.unpackbits(lsb, bitorder="little")[:150], by[:150])
    off, wr, sk = EC.encode_ref(gen, 2, 6, u, 20, EC.OPEN, 5, nout=100, offsets=[50, -1, 61])
    assert (wr, sk) == (1, 2) and np.array_equal(off[50:90], full[0]) and not off[:50].any()


# ── the library's argument checks ──

# a valid call of (133,171): five terminated frames of 100 steps at stride 203 from position 3, the
# last one ending at nout.  It is only ever sent with F = 0 or with one argument spoilt.
GOOD = dict(keep=None, period=0, info=0x10000, pitch=4, F=5, T=100, mode=1, state=0, format=2, amplitude=0, out=0x20000,
            nout=3 + 4 * 203 + 200, start=3, stride=203, offsets=None, stats=0x30000)


def call(pkg, code=None, **kw):
    a = dict(GOOD, **kw)
    code = pkg.Code(M6, 6, 1, 2) if code is None else code
    return pkg.lib().cvd_encode_frames(code.c, a["keep"], a["period"], a["info"], a["pitch"], a["F"], a["T"], a["mode"],
                                       a["state"], a["format"], a["amplitude"], a["out"], a["nout"], a["start"],
                                       a["stride"], a["offsets"], a["stats"], None)


INVALID = {
    "mode_negative": dict(mode=-1),
    "mode_three": dict(mode=3),
    "format_negative": dict(format=-1),
    "format_four": dict(format=4),
    "amplitude_in_bytes": dict(amplitude=1),
    "amplitude_in_lsb": dict(format=0, amplitude=24),
    "soft_amplitude_zero": dict(format=3, amplitude=0),
    "soft_amplitude_128": dict(format=3, amplitude=128),
    "soft_amplitude_negative": dict(format=3, amplitude=-1),
    "state_negative": dict(state=-1),
    "state_two_to_m": dict(state=64),
    "open_state_two_to_m": dict(mode=0, state=64),
    "T_zero": dict(T=0),
    "T_negative": dict(T=-1),
    "T_two_to_31": dict(T=1 << 31, pitch=1 << 26, nout=I64_MAX - 200, stride=1 << 33),
    "terminated_T_below_m": dict(T=5, stride=10, nout=3 + 4 * 10 + 10),
    "pitch_below_w": dict(pitch=3),
    "pitch_zero": dict(pitch=0),
    "F_negative": dict(F=-1),
    "nout_negative": dict(nout=-1),
    "period_17": dict(keep=bytes([3] * 17), period=17),
    "period_zero": dict(keep=bytes([3]), period=0),
    "zero_column": dict(keep=bytes([3, 0]), period=2),
    "column_bit_at_n": dict(keep=bytes([3, 4]), period=2),
    "start_negative": dict(start=-1),
    "stride_zero": dict(stride=0),
    "stride_below_span": dict(stride=199, nout=I64_MAX // 2),
    "last_frame_one_past_nout": dict(nout=GOOD["nout"] - 1),
    "one_frame_more": dict(F=6),
    "start_overflows": dict(start=I64_MAX - 100, nout=I64_MAX - 200),
    "stride_product_overflows": dict(stride=I64_MAX // 2, nout=I64_MAX - 200),
    "F_times_pitch_overflows": dict(F=1 << 40, pitch=1 << 30, offsets=0x40000),
    "nout_near_int64_max": dict(nout=I64_MAX, offsets=0x40000),
    "offsets_in_lsb": dict(format=0, offsets=0x40000),
    "offsets_in_msb": dict(format=1, offsets=0x40000),
    "null_info": dict(info=None),
    "null_out": dict(out=None),
    "misaligned_info": dict(info=0x10002),
    "misaligned_out": dict(out=0x20008),
    "misaligned_offsets": dict(offsets=0x40004),
    "misaligned_stats": dict(stats=0x30004),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_invalid_arguments(pkg, case):
    assert call(pkg, F=0) == 0             # the base arguments themselves are valid
    rc = call(pkg, **INVALID[case])
    assert rc == -1, (case, rc)
    msg = pkg.lib().cvd_last_error()
    assert msg and msg.startswith(NAME + b":"), (case, msg)


def test_no_frames_is_ok_without_a_launch(pkg):
    null = dict(info=None, out=None, stats=None)
    for mode in (0, 1, 2):
        assert call(pkg, F=0, mode=mode, **null) == 0
    for fmt, amp in ((0, 0), (1, 0), (2, 0), (3, 24), (3, 1), (3, 127)):
        assert call(pkg, F=0, format=fmt, amplitude=amp, **null) == 0
    assert call(pkg, F=0, T=0, **null) == 0                 # T is a property of the frames
    assert call(pkg, F=0, T=3, **null) == 0
    assert call(pkg, F=0, nout=0, start=0, **null) == 0
    assert call(pkg, F=0, mode=2, state=-5, **null) == 0    # tail-biting ignores start_state
    assert call(pkg, F=0, offsets=0x40000, start=-5, stride=0, **null) == 0      # offsets mode ignores both
    assert call(pkg, F=0, keep=bytes([3, 2, 1]), period=3, **null) == 0
    assert call(pkg, F=0, mode=3, **null) == -1             # the arguments are still checked


def test_unsupported_shapes(pkg):
    lib = pkg.lib()
    r23 = pkg.CONFIG_CODES["r23_m4"]
    shapes = {
        "k2": pkg.Code(r23["gen1"], 4, 2, 3),
        "n1": pkg.Code([[[1, 1, 1]]], 2, 1, 1),
        "n4": pkg.Code([[[1, 1, 1]], [[1, 0, 1]], [[1, 1, 0]], [[0, 1, 1]]], 2, 1, 4),
        "m17": pkg.Code([[[1] * 18], [[1, 0] * 9]], 17, 1, 2),
        "m0": pkg.Code([[[1]], [[1]]], 0, 1, 2),
    }
    for name, code in shapes.items():
        assert call(pkg, code=code) == -2, name
        assert lib.cvd_last_error().startswith(NAME + b":")
        assert call(pkg, code=code, F=0) == -2, name
    assert call(pkg, code=pkg.Code([[[1, 1]], [[0, 1]]], 1, 1, 2), F=0) == 0
    assert call(pkg, code=pkg.Code(EC.gen_of(16, 3), 16, 1, 3), F=0) == 0
    assert call(pkg, code=pkg.Code(EC.gen_of(9, 2), 9, 1, 2), F=0) == 0


def test_abi_and_exports(pkg):
    assert pkg.lib().cvd_version() == 11
    src = open(os.path.join(ROOT, "include", "cvd.h")).read()
    assert int(re.search(r"#define CVD_ABI_VERSION\s+(\d+)", src).group(1)) == 11
    assert "cvd_encode_frames" in pkg._lib.EXPORTS and re.search(r"\bcvd_encode_frames\(", src)
    for name, value in (("CVD_ENCODE_OPEN", 0), ("CVD_ENCODE_TERMINATED", 1), ("CVD_ENCODE_TAILBITING", 2),
                        ("CVD_CAPTURE_SOFT", 3)):
        assert int(re.search(r"#define " + name + r"\s+(\d+)", src).group(1)) == value
    enc = importlib.import_module(pkg.__name__ + ".encode")
    assert (enc.ENCODE_MODES["open"], enc.ENCODE_MODES["terminated"], enc.ENCODE_MODES["tail-biting"]) == (0, 1, 2)
    assert enc.ENCODE_FORMATS == {"lsb": 0, "msb": 1, "bytes": 2, "soft": 3} == EC.FORMATS
    for name in ("encode_frames", "encode_capture", "pack_info", "unpack_info", "encode_convolutional"):
        assert callable(getattr(pkg, name)), name
    mk = open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "Makefile")).read()
    assert "cvd_encode.o" in re.search(r"^OBJS := (.*)$", mk, re.M).group(1).split()
    assert re.search(r"^cvd_encode\.o:", mk, re.M)


# ── the Python helpers and wrappers ──

def test_pack_and_unpack_info(pkg):
    rng = np.random.default_rng(8)
    for shape in ((1,), (31,), (32,), (33,), (5, 70), (3, 64)):
        u = rng.integers(0, 2, shape).astype(np.uint8)
        rows = pkg.pack_info(u)
        T = shape[-1]
        assert rows.dtype == np.uint8 and rows.shape == shape[:-1] + ((T + 31) // 32 * 4,)
        assert np.array_equal(pkg.unpack_info(rows, T), u)
        if u.ndim == 2:
            assert np.array_equal(rows, EC.pack_rows(u))
    with pytest.raises(ValueError):
        pkg.pack_info(np.array([0, 2, 1]))


def test_wrappers_refuse_bad_arguments(pkg):
    """Every check here comes before the library or the device is asked for anything."""
    cpu = importlib.import_module("torch").device("cpu")
    info = np.zeros((4, 8), np.uint8)
    for kw in (dict(T=0), dict(T=1 << 31), dict(T=65), dict(T=40, F=5), dict(T=40, mode="closed"),
               dict(T=40, format="nibbles"), dict(T=40, amplitude=24), dict(T=40, format="soft", amplitude=0),
               dict(T=40, format="soft", amplitude=128), dict(T=40, keep="101/11"), dict(T=40, keep=[3, 0]),
               dict(T=40, offsets=np.zeros(4)), dict(T=40, offsets=np.zeros(3, np.int64)), dict(T=40, offsets=[0, 80])):
        with pytest.raises((ValueError, TypeError)):
            pkg.encode_frames(2, 6, M6, info, device=cpu, **kw)
    with pytest.raises(TypeError):
        pkg.encode_frames(2, 6, M6, info.astype(np.int8), 40, device=cpu)
    with pytest.raises(ValueError):
        pkg.encode_frames(2, 6, M6, np.zeros((4, 6), np.uint8), 40, device=cpu)      # rows of whole words
    for kw in (dict(T=0), dict(T=65), dict(format="soft", amplitude=200)):
        with pytest.raises(ValueError):
            pkg.encode_capture(2, 6, M6, np.zeros(8, np.uint8), device=cpu, **kw)
    for gens, m in (([[[1, 1, 1]]], 2), ([[[1, 1, 1]]] * 4, 2), ([[[1, 1, 1], [1, 0, 1]]] * 2, 2),
                    ([[[1] * 18]] * 2, 17), ([[[1, 1, 1, 1]], [[1, 0, 1]]], 2)):
        with pytest.raises(ValueError):
            pkg.encode_convolutional([1, 0, 1], gens, m)


# ── the shapes of the GPU round trips through the tail-biting decoders ──

def test_tailbiting_round_trip_shapes_decode_cleanly():
    """Noiseless tail-biting frames of the shapes tests/test_gpu_encode.py sends through
    decode_frames_tailbiting: the tests' host decoder returns status 0, distance 0 and s_0 = s_T on
    every frame, with a path whose codeword is the one sent (the bits themselves may differ: a
    tail-biting code at small T need not be injective)."""
    for i, (m, n, T, F, keep) in enumerate(EC.TB_ROUNDTRIP):
        gen = EC.gen_of(m, n)
        u = EC.tb_roundtrip_data(i)
        y = TG.encode_circular(n, m, gen, u.astype(np.int64))
        masks = None if keep is None else np.array([keep[t % len(keep)] for t in range(T)])
        bits, rec, words, _ = TG.ref_tailbiting(n, m, gen, TG.hard_cost(n, y, masks), 4)
        assert (rec[:, 3] == 0).all() and (rec[:, 0] == 0).all() and (rec[:, 1] == rec[:, 2]).all(), (m, n, T)
        for f in range(F):
            assert np.array_equal(EC.frame_bits(gen, n, m, bits[f], T, EC.TAILBITING, keep=keep),
                                  EC.frame_bits(gen, n, m, u[f], T, EC.TAILBITING, keep=keep)), (m, n, T, f)


def test_frame_round_trip_shapes_decode_to_the_sent_bits():
    """Noiseless terminated and open frames and the stream of the shapes the GPU round trips use:
    the tests' host decoder (test_gpu_decode_frames.ref_decode) returns the sent bits at distance 0
    with the boundary states the GPU test states."""
    for i, (m, n, T, F, keep) in enumerate(EC.RT_FRAMES):
        gen = EC.gen_of(m, n)
        masks = None if keep is None else np.array([keep[t % len(keep)] for t in range(T)])
        for mode, s0_known, end in ((EC.TERMINATED, True, 0), (EC.OPEN, True, None), (EC.OPEN, False, None)):
            u, s0 = EC.rt_data(i, mode)
            if not s0_known:
                if i not in EC.RT_STREAMS:
                    continue
                u = u[:1]                                         # the stream: one row, neither state told
            y = np.stack([(LC.encode(gen, n, m, u[f], s0)[0].reshape(T, n).astype(np.int64)
                           << np.arange(n)[None, :]).sum(axis=1) for f in range(len(u))])
            bits, dist, sa, sb, _ = TF.ref_decode(n, m, gen, TF.hard_cost(n, y, masks), s0 if s0_known else None, end)
            assert np.array_equal(bits, u) and not dist.any() and (sa == s0).all(), (m, n, T, mode, s0_known)
            assert np.array_equal(sb, [LC.encode(gen, n, m, u[f], s0)[1] for f in range(len(u))])


def test_noisy_tailbiting_frames_mostly_close():
    """The BSC(0.02) tail-biting frames of the GPU re-encode test: the reference decoder leaves at
    most 10% of them without a tail-biting survivor (status 3)."""
    for i, (m, n, T, F) in enumerate(EC.TB_NOISY):
        gen = EC.gen_of(m, n)
        _, _, recv = EC.noisy_frames(gen, n, m, T, F, EC.TAILBITING, EC.NOISY_SEED + i)
        y = (recv.reshape(F, T, n).astype(np.int64) << np.arange(n)[None, None, :]).sum(axis=2)
        _, rec, _, _ = TG.ref_tailbiting(n, m, gen, TG.hard_cost(n, y), 4)
        frac = float((rec[:, 3] == 3).mean())
        print(f"m={m} n={n} T={T}: {frac:.3f} of {F} frames have status 3")
        assert frac <= 0.10
        soft = EC.noisy_soft(recv, EC.NOISY_SEED + 40 + i).reshape(F, T, n)
        _, rec, _, _ = TG.ref_tailbiting(n, m, gen, TG.soft_cost(n, soft), 4)
        frac = float((rec[:, 3] == 3).mean())
        print(f"m={m} n={n} T={T} soft: {frac:.3f} of {F} frames have status 3")
        assert frac <= 0.10


# ── the command line ──

@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module(pkg.__name__ + ".__main__")


def test_cli_parses_encode(cli):
    a = cli.parse_args(["encode", "--code", "oct:133,171", "--input", "decoded.npy", "--frame", "128", "--tail-biting",
                        "--puncture", "dvb:3/4", "--format", "soft", "--amplitude", "7"])
    assert (a.cmd, a.frame, a.tail_biting, a.open, a.puncture, a.format, a.amplitude, a.start_state, a.T) == \
        ("encode", 128, True, False, "dvb:3/4", "soft", 7, None, None)
    a = cli.parse_args(["encode", "--code", "m6", "--input", "decoded.npy", "--T", "1000", "--start-state", "5"])
    assert (a.frame, a.T, a.start_state, a.format, a.amplitude, a.output) == (None, 1000, 5, "bytes", None, None)


@pytest.mark.parametrize("args,message", [
    (["--amplitude", "24"], "--amplitude needs --format soft"),
    (["--format", "lsb", "--amplitude", "24"], "--amplitude needs --format soft"),
    (["--format", "soft", "--amplitude", "0"], "--amplitude takes 1..127"),
    (["--format", "soft", "--amplitude", "128"], "--amplitude takes 1..127"),
    (["--frame", "64", "--tail-biting", "--start-state", "0"], "--tail-biting does not go with --start-state"),
    (["--frame", "64", "--tail-biting", "--open"], "--open and --tail-biting exclude one another"),
    (["--frame", "64", "--T", "64"], "it does not go with --T"),
    (["--frame-count", "3"], "need --frame"),
    (["--frame-stride", "200"], "need --frame"),
    (["--open"], "need --frame"),
    (["--tail-biting"], "need --frame"),
    (["--start-state", "-1"], "a state number is not negative"),
    (["--format", "nibbles"], "argument --format: invalid choice: 'nibbles'"),
])
def test_cli_encode_argument_errors(cli, capsys, args, message):
    with pytest.raises(SystemExit):
        cli.parse_args(["encode", "--code", "m6", "--input", "decoded.npy"] + args)
    err = capsys.readouterr().err
    assert "encode" in err and message in err, err


def test_cli_encode_needs_code_and_input(cli, capsys):
    for args, missing in ((["--input", "decoded.npy"], "--code"), (["--code", "m6"], "--input")):
        with pytest.raises(SystemExit):
            cli.parse_args(["encode"] + args)
        err = capsys.readouterr().err
        assert " encode: error: the following arguments are required: " + missing in err, err

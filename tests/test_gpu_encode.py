"""cvd_encode_frames on the GPU against the sequential encoder of encode_cases.py (written from
include/cvd.h): the whole output buffer, zeros and padding included, compared exactly in every
format, with a canary behind the rounded length; then the round trips through the public decoders
(noiseless: the sent bits, or the sent codeword for tail-biting frames, at distance 0; noisy:
re-encoding the decoded bits and comparing with the capture counts exactly the errors that the
decoder reports), the command line and parity.encode_convolutional."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import encode_cases as EC
import llr_cases as LC

pytestmark = pytest.mark.gpu

CANARY = 0xA5
DVB = ["dvb:2/3", "dvb:3/4", "dvb:5/6", "dvb:7/8"]
P16 = {2: [1, 2, 3, 1, 1, 2, 2, 3, 1, 3, 2, 1, 1, 1, 2, 3], 3: [1, 2, 4, 7, 3, 5, 6, 1, 1, 2, 4, 4, 7, 3, 1, 2]}


def raw_encode(pkg, gen, n, m, rows, T, mode, state=0, keep=None, format="bytes", amplitude=0, nout=None, start=0,
               stride=None, offsets=None, F=None, pitch=None):
    """cvd_encode_frames itself on `rows` (numpy uint8 [F, 4*pitch], or a device tensor whose row
    pitch is given): (the whole buffer up to the rounded length as numpy uint8, written, skipped).
    The buffer is allocated 64 bytes longer and pre-filled: the bytes behind the rounded length
    must come back untouched, and every byte before it must have been written."""
    dev = torch.device("cuda", 0)
    code = pkg.Code(gen, m, 1, n)
    if isinstance(rows, np.ndarray):
        F, pitch = rows.shape[0], rows.shape[1] // 4
        rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    span = EC.span_of(n, T, keep)
    stride = span if stride is None else stride
    off = None
    if offsets is not None:
        off = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).to(dev)
    elif nout is None:
        nout = start + (F - 1) * stride + span
    fmt = EC.FORMATS[format]
    nbytes = nout if fmt in (EC.BYTES, EC.SOFT) else (nout + 7) // 8
    rounded = (nbytes + 15) // 16 * 16
    out = torch.full((rounded + 64,), CANARY, dtype=torch.uint8, device=dev)
    stats = torch.full((2,), -7, dtype=torch.int64, device=dev)
    rc = pkg.lib().cvd_encode_frames(code.c, bytes(keep) if keep else None, len(keep) if keep else 0,
                                     ctypes.c_void_p(rows.data_ptr()), pitch, F, T, mode, state, fmt, amplitude,
                                     ctypes.c_void_p(out.data_ptr()), nout, start, stride,
                                     ctypes.c_void_p(off.data_ptr()) if off is not None else None,
                                     ctypes.c_void_p(stats.data_ptr()), None)
    assert rc == 0, pkg.lib().cvd_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[rounded:] == CANARY).all(), "bytes at or past the rounded length were written"
    s = stats.cpu().tolist()
    return got[:rounded], s[0], s[1]


def check(pkg, gen, n, m, u, T, mode, rng=None, pitch=None, **kw):
    """One call against the reference, on rows packed from u [F, T] (bits at or past T random when
    an rng is given)."""
    rows = EC.pack_rows(u, pitch, fill=rng)
    got, wr, sk = raw_encode(pkg, gen, n, m, rows, T, mode, **kw)
    ref = dict(kw)
    ref["start_state"] = ref.pop("state", 0)
    want, wwr, wsk = EC.encode_ref(gen, n, m, u, T, mode, **ref)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (m, n, T, mode, kw, np.flatnonzero(got != want)[:10])
    assert (wr, sk) == (wwr, wsk)


# ── every code, T, mode and start state ──

@pytest.mark.parametrize("m,n", EC.ALL_CODES)
def test_codes_lengths_modes(pkg, m, n):
    gen = EC.gen_of(m, n)
    rng = np.random.default_rng(1000 * m + n)
    formats = ["bytes", "lsb", "soft", "msb"]
    i = 0
    for T in sorted({1, m - 1, m, m + 1, 31, 32, 33, 63, 64, 65, 127, 129} - {0}):
        w = (T + 31) // 32
        u = rng.integers(0, 2, (3, T)).astype(np.uint8)                 # terminated: garbage in the last m bits
        for mode in (EC.OPEN, EC.TERMINATED, EC.TAILBITING):
            if mode == EC.TERMINATED and T < m:
                continue
            states = [0] if mode == EC.TAILBITING else [0, 1, (1 << m) - 1, int(rng.integers(1 << m))]
            for state in states:
                fmt = formats[i % 4]
                i += 1
                check(pkg, gen, n, m, u, T, mode, rng=rng, pitch=w + (i % 3 == 0), state=state, format=fmt,
                      amplitude=24 if fmt == "soft" else 0, start=i % 5, stride=EC.span_of(n, T) + i % 7)


def test_formats(pkg):
    gen, rng = EC.gen_of(6, 2), np.random.default_rng(2)
    u = rng.integers(0, 2, (5, 65)).astype(np.uint8)
    kw = dict(state=37, start=3, stride=135, nout=3 + 4 * 135 + 130 + 9)
    check(pkg, gen, 2, 6, u, 65, EC.OPEN, format="bytes", **kw)
    check(pkg, gen, 2, 6, u, 65, EC.OPEN, format="lsb", **kw)
    check(pkg, gen, 2, 6, u, 65, EC.OPEN, format="msb", **kw)
    for A in (1, 24, 127):
        check(pkg, gen, 2, 6, u, 65, EC.OPEN, format="soft", amplitude=A, **kw)
    by, _, _ = raw_encode(pkg, gen, 2, 6, EC.pack_rows(u), 65, EC.OPEN, format="bytes", **kw)
    msb, _, _ = raw_encode(pkg, gen, 2, 6, EC.pack_rows(u), 65, EC.OPEN, format="msb", **kw)
    packed = np.packbits(by[:kw["nout"]])                               # numpy's default bit order
    assert np.array_equal(msb[:len(packed)], packed) and not msb[len(packed):].any()


@pytest.mark.parametrize("n", [2, 3])
def test_patterns(pkg, n):
    gen, rng = EC.gen_of(6, n), np.random.default_rng(3 + n)
    dec = importlib.import_module(pkg.__name__ + ".decode")
    pats = [P16[n]] + ([dec.puncture_pattern(p, 2) for p in DVB] if n == 2 else [])
    formats = ["bytes", "lsb", "soft", "msb"]
    i = 0
    for keep in pats:
        for T in (1, 5, 16, 33, 100, 129):
            u = rng.integers(0, 2, (4, T)).astype(np.uint8)
            for mode in (EC.OPEN, EC.TERMINATED, EC.TAILBITING):
                if mode == EC.TERMINATED and T < 6:
                    continue
                fmt = formats[i % 4]
                i += 1
                check(pkg, gen, n, 6, u, T, mode, rng=rng, keep=keep, state=0 if mode == EC.TAILBITING else 41, format=fmt,
                      amplitude=9 if fmt == "soft" else 0, start=i % 4, stride=EC.span_of(n, T, keep) + (i % 3) * 17)
    # all-kept patterns are no puncturing
    u = rng.integers(0, 2, (4, 70)).astype(np.uint8)
    for fmt in ("bytes", "lsb"):
        plain, _, _ = raw_encode(pkg, gen, n, 6, EC.pack_rows(u), 70, EC.TERMINATED, format=fmt, start=5, stride=n * 70 + 3)
        for period in (1, 5):
            kept, _, _ = raw_encode(pkg, gen, n, 6, EC.pack_rows(u), 70, EC.TERMINATED, keep=[(1 << n) - 1] * period,
                                    format=fmt, start=5, stride=n * 70 + 3)
            assert np.array_equal(kept, plain)
            check(pkg, gen, n, 6, u, 70, EC.TERMINATED, keep=[(1 << n) - 1] * period, format=fmt, start=5, stride=n * 70 + 3)


# ── placement ──

@pytest.mark.parametrize("format", ["lsb", "msb", "bytes", "soft"])
def test_stride_placement(pkg, format):
    gen, rng = EC.gen_of(6, 2), np.random.default_rng(4)
    amp = 24 if format == "soft" else 0
    u = rng.integers(0, 2, (9, 37)).astype(np.uint8)
    for start in (0, 3, 37):
        for gap in (0, 1, 5, 31, 32, 33):
            check(pkg, gen, 2, 6, u, 37, EC.TAILBITING, format=format, amplitude=amp, start=start, stride=74 + gap,
                  nout=start + 8 * (74 + gap) + 74 + (start + gap) % 3 * 50)
    # span 2 at stride 2: sixteen frames in a word; and at stride 3, with gaps inside every word
    g1 = EC.gen_of(1, 2)
    u1 = rng.integers(0, 2, (300, 1)).astype(np.uint8)
    for stride in (2, 3):
        for mode, state in ((EC.OPEN, 1), (EC.TAILBITING, 0)):
            check(pkg, g1, 2, 1, u1, 1, mode, state=state, format=format, amplitude=amp, start=1, stride=stride)
    check(pkg, g1, 2, 1, u1, 1, EC.TERMINATED, format=format, amplitude=amp, stride=2)     # T = m: every input is tail
    # a single frame ending mid-word, and one with room behind it
    one = rng.integers(0, 2, (1, 45)).astype(np.uint8)
    check(pkg, gen, 2, 6, one, 45, EC.OPEN, state=5, format=format, amplitude=amp)
    check(pkg, gen, 2, 6, one, 45, EC.OPEN, state=5, format=format, amplitude=amp, start=7, nout=400, stride=1 << 40)


@pytest.mark.parametrize("format", ["bytes", "soft"])
def test_offsets_placement(pkg, format):
    rng = np.random.default_rng(5)
    amp = 127 if format == "soft" else 0
    for n, keep in ((2, None), (3, None), (2, [3, 2, 1]), (3, P16[3])):
        gen = EC.gen_of(6, n)
        T = 41
        span = EC.span_of(n, T, keep)
        u = rng.integers(0, 2, (9, T)).astype(np.uint8)
        nout = 6 * span + 200
        # unsorted, with gaps; frames 1, 4, 6, 8 lie outside at either end (by one position, or wholly)
        offsets = np.array([3 * span + 70, -1, 5, nout - span, nout - span + 1, 2 * span + 33, -span - 5, span + 6, nout + 3])
        check(pkg, gen, n, 6, u, T, EC.TERMINATED, rng=rng, keep=keep, format=format, amplitude=amp, nout=nout,
              offsets=offsets)
        rows = EC.pack_rows(u)
        _, wr, sk = raw_encode(pkg, gen, n, 6, rows, T, EC.TERMINATED, keep=keep, format=format, amplitude=amp, nout=nout,
                               offsets=offsets)
        assert (wr, sk) == (5, 4)
        # every frame skipped: the capture is all zeros
        got, wr, sk = raw_encode(pkg, gen, n, 6, rows, T, EC.TERMINATED, keep=keep, format=format, amplitude=amp,
                                 nout=span - 1, offsets=np.zeros(9, np.int64))
        assert (wr, sk) == (0, 9) and not got.any()


# ── launch shape ──

@pytest.fixture(scope="module")
def long_stream():
    """A stream over a few launch tiles with a ragged end, and its reference, made once."""
    gen, rng = EC.gen_of(6, 2), np.random.default_rng(6)
    T = 20011
    u = rng.integers(0, 2, (1, T)).astype(np.uint8)
    want = {}
    for fmt, keep in (("bytes", None), ("lsb", None), ("soft", [3, 2, 1]), ("msb", [3, 2, 1])):
        want[(fmt, keep is None)] = EC.encode_ref(gen, 2, 6, u, T, EC.OPEN, 19, keep, fmt, 24 if fmt == "soft" else 0)[0]
    for w in want.values():
        w.setflags(write=False)
    return gen, T, EC.pack_rows(u), want


@pytest.mark.parametrize("blocks", [None, "1", "3"])
def test_long_stream_any_launch_shape(pkg, long_stream, monkeypatch, blocks):
    gen, T, rows, want = long_stream
    if blocks is None:
        monkeypatch.delenv("CVD_ENCODE_BLOCKS", raising=False)
    else:
        monkeypatch.setenv("CVD_ENCODE_BLOCKS", blocks)
    for (fmt, plain), w in want.items():
        got, wr, sk = raw_encode(pkg, gen, 2, 6, rows, T, EC.OPEN, state=19, keep=None if plain else [3, 2, 1], format=fmt,
                                 amplitude=24 if fmt == "soft" else 0)
        assert np.array_equal(got, w), (fmt, plain, blocks, np.flatnonzero(got != w)[:10])
        assert (wr, sk) == (1, 0)


def test_many_frames_grid_stride_and_offsets(pkg, monkeypatch):
    """Frames over several blocks, also in offsets mode, at a capped launch."""
    gen, rng = EC.gen_of(6, 3), np.random.default_rng(7)
    T, F = 24, 400
    u = rng.integers(0, 2, (F, T)).astype(np.uint8)
    offsets = rng.permutation(F).astype(np.int64) * 80 + 3
    for blocks in ("2", None):
        if blocks is None:
            monkeypatch.delenv("CVD_ENCODE_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("CVD_ENCODE_BLOCKS", blocks)
        check(pkg, gen, 3, 6, u, T, EC.TAILBITING, format="soft", amplitude=24, nout=80 * F + 10, offsets=offsets)
        check(pkg, gen, 3, 6, u, T, EC.TAILBITING, format="lsb", start=3, stride=80)


# ── the Python interface ──

def test_python_interface(pkg):
    gen, rng = EC.gen_of(6, 2), np.random.default_rng(8)
    T, F, L = 50, 6, 3
    w = (T + 31) // 32
    u = rng.integers(0, 2, (F, L, T)).astype(np.uint8)
    lists = np.stack([EC.pack_rows(u[:, i], fill=rng) for i in range(L)], axis=1)        # [F, L, 4w] as a list result
    dev_lists = torch.from_numpy(lists).cuda()
    for i in range(L):
        view = dev_lists[:, i]
        assert not view.is_contiguous() or L == 1
        res = pkg.encode_frames(2, 6, gen, view, T, mode="tail-biting", format="lsb", start=5)
        want, _, _ = EC.encode_ref(gen, 2, 6, u[:, i], T, EC.TAILBITING, format="lsb", start=5)
        assert res["capture"].dtype == torch.uint8 and res["nbits"] == 5 + F * 100
        assert (res["span"], res["stride"], res["F"], res["T"], res["written"], res["skipped"]) == (100, 100, F, T, F, 0)
        got = res["capture"].cpu().numpy()
        assert np.array_equal(got, want[:len(got)]) and len(got) == (res["nbits"] + 7) // 8
    # numpy rows, soft, a pattern, an explicit size; pack_info's rows
    res = pkg.encode_frames(2, 6, gen, pkg.pack_info(u[:, 0]), T, keep="dvb:3/4", format="soft", amplitude=7, stride=70,
                            size=500)
    want, _, _ = EC.encode_ref(gen, 2, 6, u[:, 0], T, EC.TERMINATED, keep=[3, 2, 1], format="soft", amplitude=7, stride=70,
                               nout=500)
    assert res["capture"].dtype == torch.int8 and res["span"] == EC.span_of(2, T, [3, 2, 1]) and res["nbits"] == 500
    assert np.array_equal(res["capture"].cpu().numpy().view(np.uint8), want[:500])
    # offsets through the wrapper
    offsets = np.array([300, -4, 0, 150, 1000, 75], np.int64)
    res = pkg.encode_frames(2, 6, gen, pkg.pack_info(u[:, 1]), 30, mode="open", start_state=9, offsets=offsets, size=400)
    want, wr, sk = EC.encode_ref(gen, 2, 6, u[:, 1], 30, EC.OPEN, 9, nout=400, offsets=offsets)
    assert (res["written"], res["skipped"]) == (wr, sk) == (4, 2)
    assert np.array_equal(res["capture"].cpu().numpy(), want[:400])
    # the stream: any number of bytes, the end state continues it
    bits = rng.integers(0, 2, 203).astype(np.uint8)
    packed = np.packbits(bits, bitorder="little")
    a = pkg.encode_capture(2, 6, gen, packed, T=120, start_state=33)
    b = pkg.encode_capture(2, 6, gen, np.packbits(bits[120:], bitorder="little"), T=83, start_state=a["end_state"])
    whole, end = LC.encode(gen, 2, 6, bits, 33)
    assert np.array_equal(np.concatenate([a["capture"].cpu().numpy(), b["capture"].cpu().numpy()]), whole)
    assert b["end_state"] == end and a["nbits"] == 240
    short = pkg.encode_capture(2, 6, gen, packed, T=3, start_state=33)
    assert short["end_state"] == LC.encode(gen, 2, 6, bits[:3], 33)[1]
    empty = pkg.encode_frames(2, 6, gen, np.zeros((0, 8), np.uint8), 40)
    assert empty["F"] == 0 and empty["written"] == 0 and empty["nbits"] == 0


def test_encode_convolutional_matches_the_golden_pairs(pkg):
    for name, gen, m, u, v in EC.golden_pairs():
        got = pkg.encode_convolutional(u.tolist(), gen, m)
        assert isinstance(got, list) and np.array_equal(np.array(got), v), name


# ── round trips through the public decoders, noiseless ──

@pytest.mark.parametrize("i", range(len(EC.RT_FRAMES)))
def test_round_trip_frames(pkg, i):
    m, n, T, F, keep = EC.RT_FRAMES[i]
    gen = EC.gen_of(m, n)
    span = EC.span_of(n, T, keep)
    for mode, name in ((EC.TERMINATED, "terminated"), (EC.OPEN, "open")):
        u, s0 = EC.rt_data(i, mode)
        ends = [LC.encode(gen, n, m, u[f], s0)[1] for f in range(F)]
        rows = pkg.pack_info(u)
        for fmt in ("bytes", "lsb", "msb"):
            enc = pkg.encode_frames(n, m, gen, rows, T, mode=name, start_state=s0, keep=keep, format=fmt, start=3,
                                    stride=span + 5)
            res = pkg.decode_frames(n, m, gen, enc["capture"], T, F=F, start=3, stride=span + 5, start_state=s0,
                                    end_state=0 if mode == EC.TERMINATED else None, keep=keep, format=fmt, nbits=enc["nbits"])
            assert np.array_equal(res["bits"].cpu().numpy(), rows), (m, n, T, name, fmt)
            assert res["total_distance"] == 0 and res["decoded"] == F and res["total_counted"] == F * span
            assert res["start_states"].cpu().tolist() == [s0] * F and res["end_states"].cpu().tolist() == ends
        soft = pkg.encode_frames(n, m, gen, rows, T, mode=name, start_state=s0, keep=keep, format="soft", amplitude=24,
                                 start=3, stride=span + 5)
        kw = dict(F=F, start=3, stride=span + 5, start_state=s0, end_state=0 if mode == EC.TERMINATED else None)
        if keep is None:
            res = pkg.decode_frames_soft(n, m, gen, soft["capture"], T, **kw)
        else:
            res = pkg.decode_frames_soft_punctured(n, m, gen, keep, soft["capture"], T, **kw)
        assert np.array_equal(res["bits"].cpu().numpy(), rows)
        assert res["total_distance"] == 0 and res["total_errors"] == 0
        assert res["counted"].cpu().tolist() == [span] * F                # gaps are erasures, frames have none
    if i in EC.RT_STREAMS:
        u, s0 = EC.rt_data(i, EC.OPEN)
        packed = pkg.pack_info(u[0])
        enc = pkg.encode_capture(n, m, gen, packed, T=T, start_state=s0, keep=keep, format="msb")
        if keep is None:
            res = pkg.decode_capture(n, m, gen, enc["capture"], T=T, format="msb", nbits=enc["nbits"])
        else:
            res = pkg.decode_capture_punctured(n, m, gen, keep, enc["capture"], T=T, format="msb", nbits=enc["nbits"])
        assert np.array_equal(res["bits"].cpu().numpy(), packed) and res["errors"] == 0
        assert (res["start_state"], res["end_state"]) == (s0, enc["end_state"])


@pytest.mark.parametrize("i", range(len(EC.TB_ROUNDTRIP)))
def test_round_trip_tailbiting(pkg, i):
    m, n, T, F, keep = EC.TB_ROUNDTRIP[i]
    gen = EC.gen_of(m, n)
    u = EC.tb_roundtrip_data(i)
    span = EC.span_of(n, T, keep)
    enc = pkg.encode_frames(n, m, gen, pkg.pack_info(u), T, mode="tail-biting", keep=keep, format="lsb", stride=span + 1)
    res = pkg.decode_frames_tailbiting(n, m, gen, enc["capture"], T, F=F, stride=span + 1, keep=keep, format="lsb",
                                       nbits=enc["nbits"])
    assert res["status"].cpu().tolist() == [0] * F and res["total_distance"] == 0
    assert torch.equal(res["start_states"], res["end_states"])
    again = pkg.encode_frames(n, m, gen, res["bits"], T, mode="tail-biting", keep=keep, format="lsb", stride=span + 1)
    assert torch.equal(again["capture"], enc["capture"])                  # the codeword, not necessarily the bits
    soft = pkg.encode_frames(n, m, gen, pkg.pack_info(u), T, mode="tail-biting", keep=keep, format="soft", amplitude=3)
    if keep is None:
        res = pkg.decode_frames_tailbiting_soft(n, m, gen, soft["capture"], T, F=F)
    else:
        res = pkg.decode_frames_tailbiting_soft_punctured(n, m, gen, keep, soft["capture"], T, F=F)
    assert res["status"].cpu().tolist() == [0] * F and res["total_distance"] == 0
    assert res["counted"].cpu().tolist() == [span] * F
    again = pkg.encode_frames(n, m, gen, res["bits"], T, mode="tail-biting", keep=keep, format="soft", amplitude=3)
    assert torch.equal(again["capture"], soft["capture"])


# ── re-encoding what was decoded shows where the channel errors are ──

def test_reencode_identity_terminated(pkg):
    m, n, T, F = 6, 2, 64, 96
    gen = EC.gen_of(m, n)
    _, sent, recv = EC.noisy_frames(gen, n, m, T, F, EC.TERMINATED, EC.NOISY_SEED + 20)
    assert (sent != recv).any()
    res = pkg.decode_frames(n, m, gen, recv.reshape(-1), T, F=F)
    enc = pkg.encode_frames(n, m, gen, res["bits"], T, mode="terminated")
    diff = (enc["capture"].cpu().numpy().reshape(F, n * T) != recv).sum(axis=1)
    assert np.array_equal(diff, res["distance"].cpu().numpy())
    assert int(diff.sum()) == res["total_errors"] > 0
    # soft, with erasures: the sign disagreements at the values that are not 0
    soft = EC.noisy_soft(recv, EC.NOISY_SEED + 21)
    res = pkg.decode_frames_soft(n, m, gen, soft.reshape(-1), T, F=F)
    enc = pkg.encode_frames(n, m, gen, res["bits"], T, mode="terminated", format="soft", amplitude=24)
    again = enc["capture"].cpu().numpy().reshape(F, n * T)
    diff = ((soft != 0) & ((soft > 0) != (again > 0))).sum(axis=1)
    assert np.array_equal(diff, res["errors"].cpu().numpy()) and int(diff.sum()) == res["total_errors"] > 0


@pytest.mark.parametrize("i", range(len(EC.TB_NOISY)))
def test_reencode_identity_tailbiting(pkg, i):
    m, n, T, F = EC.TB_NOISY[i]
    gen = EC.gen_of(m, n)
    _, sent, recv = EC.noisy_frames(gen, n, m, T, F, EC.TAILBITING, EC.NOISY_SEED + i)
    res = pkg.decode_frames_tailbiting(n, m, gen, recv.reshape(-1), T, F=F)
    status = res["status"].cpu().numpy()
    closed = (status == 0) | (status == 2)
    left_out = int((status == 3).sum())
    print(f"m={m} n={n} T={T}: {left_out} of {F} frames have status 3 and are left out")
    assert closed.sum() + left_out == F and left_out <= F // 10
    enc = pkg.encode_frames(n, m, gen, res["bits"], T, mode="tail-biting")
    diff = (enc["capture"].cpu().numpy().reshape(F, n * T) != recv).sum(axis=1)
    assert np.array_equal(diff[closed], res["distance"].cpu().numpy()[closed]) and diff[closed].sum() > 0
    # soft, with erasures: the sign disagreements at the values that are not 0
    soft = EC.noisy_soft(recv, EC.NOISY_SEED + 40 + i)
    res = pkg.decode_frames_tailbiting_soft(n, m, gen, soft.reshape(-1), T, F=F)
    status = res["status"].cpu().numpy()
    closed = (status == 0) | (status == 2)
    left_out = int((status == 3).sum())
    print(f"m={m} n={n} T={T} soft: {left_out} of {F} frames have status 3 and are left out")
    assert closed.sum() + left_out == F and left_out <= F // 10
    enc = pkg.encode_frames(n, m, gen, res["bits"], T, mode="tail-biting", format="soft", amplitude=24)
    again = enc["capture"].cpu().numpy().reshape(F, n * T)
    diff = ((soft != 0) & ((soft > 0) != (again > 0))).sum(axis=1)
    assert np.array_equal(diff[closed], res["errors"].cpu().numpy()[closed]) and diff[closed].sum() > 0


# ── the command line ──

def test_cli_decode_then_encode_gives_the_file_back(pkg, tmp_path, capsys):
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    gen, rng = EC.gen_of(6, 2), np.random.default_rng(9)
    # a stream
    bits = rng.integers(0, 2, 1000).astype(np.uint8)
    cap = np.packbits(LC.encode(gen, 2, 6, bits, 0)[0])                               # --format msb
    np.save(tmp_path / "stream.npy", cap)
    assert cli.main(["decode", "--code", "oct:133,171", "--input", str(tmp_path / "stream.npy"), "--format", "msb",
                     "--save-dir", str(tmp_path)]) == 0
    assert cli.main(["encode", "--code", "oct:133,171", "--input", str(tmp_path / "decoded.npy"), "--T", "1000",
                     "--format", "msb", "--output", str(tmp_path / "again.npy")]) == 0
    assert np.array_equal(np.load(tmp_path / "again.npy"), cap)
    assert "span 2000 bits" in capsys.readouterr().out
    # punctured terminated frames, one bit per byte, with a gap between them
    u, _ = EC.rt_data(5, EC.TERMINATED)
    keep = EC.RT_FRAMES[5][4]
    frames, _, _ = EC.encode_ref(gen, 2, 6, u, 60, EC.TERMINATED, keep=keep, stride=85)
    frames = frames[:7 * 85 + 80]
    np.save(tmp_path / "frames.npy", frames)
    assert cli.main(["decode", "--code", "oct:133,171", "--input", str(tmp_path / "frames.npy"), "--frame", "60",
                     "--frame-stride", "85", "--puncture", "101/110", "--save-dir", str(tmp_path)]) == 0
    assert cli.main(["encode", "--code", "oct:133,171", "--input", str(tmp_path / "decoded.npy"), "--frame", "60",
                     "--frame-stride", "85", "--puncture", "101/110", "--save-dir", str(tmp_path)]) == 0
    assert np.array_equal(np.load(tmp_path / "encoded.npy"), frames)
    # tail-biting soft frames
    ut = EC.tb_roundtrip_data(1)
    soft = EC.encode_ref(gen, 2, 6, ut, 40, EC.TAILBITING, format="soft", amplitude=5)[0][:16 * 80].view(np.int8)
    np.save(tmp_path / "soft.npy", soft)
    assert cli.main(["decode", "--code", "m6", "--input", str(tmp_path / "soft.npy"), "--format", "soft", "--frame", "40",
                     "--tail-biting", "--save-dir", str(tmp_path)]) == 0
    assert cli.main(["encode", "--code", "m6", "--input", str(tmp_path / "decoded.npy"), "--frame", "40", "--tail-biting",
                     "--format", "soft", "--amplitude", "5", "--save-dir", str(tmp_path)]) == 0
    assert np.array_equal(np.load(tmp_path / "encoded.npy"), soft)

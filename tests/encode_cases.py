"""A sequential encoder written from include/cvd.h's text of cvd_encode_frames: a state walk
step by step, every mode, the pattern and the placement, producing the whole expected output
buffer in each format (zeros and padding included).  The reference of the encoder's tests."""
import numpy as np

import llr_cases as LC

OPEN, TERMINATED, TAILBITING = 0, 1, 2
LSB, MSB, BYTES, SOFT = 0, 1, 2, 3
FORMATS = {"lsb": LSB, "msb": MSB, "bytes": BYTES, "soft": SOFT}
MODES = {"open": OPEN, "terminated": TERMINATED, "tail-biting": TAILBITING}

# the decoders' code list, and fixed random taps past it (delay-0 and delay-m taps set)
DECODER_SHAPES = [(1, 2), (2, 2), (5, 2), (6, 2), (6, 3), (7, 2), (8, 2), (8, 3)]
DECODER_GENS = {mn: LC.gen_of(*mn) for mn in DECODER_SHAPES}


def random_gen(m, n, seed=2024):
    rng = np.random.default_rng(seed + 100 * m + n)
    gen = []
    for _ in range(n):
        t = rng.integers(0, 2, m + 1)
        t[0] = t[m] = 1
        gen.append([[int(b) for b in t]])
    return gen


def gen_of(m, n):
    return DECODER_GENS[(m, n)] if (m, n) in DECODER_GENS else random_gen(m, n)


ALL_CODES = sorted(DECODER_GENS) + [(m, n) for m in (9, 15, 16) for n in (2, 3)]


def pack_rows(u, pitch=None, fill=None):
    """0/1 array [F, T] -> uint8 [F, 4*pitch], bit t of row f LSB first; the bits at or past T
    (and the words past ceil(T/32)) are zero, or random from the generator `fill`."""
    u = np.asarray(u, np.uint8)
    F, T = u.shape
    w = (T + 31) // 32
    pitch = w if pitch is None else pitch
    full = np.zeros((F, 32 * pitch), np.uint8) if fill is None else fill.integers(0, 2, (F, 32 * pitch)).astype(np.uint8)
    full[:, :T] = u
    return np.packbits(full, axis=1, bitorder="little")


def frame_bits(gen, n, m, u, T, mode, start_state=0, keep=None):
    """The emitted bits of one frame (the kept outputs, in order) from the row's bits u[0..T)."""
    u = [int(b) for b in u[:T]]
    if mode == TERMINATED:
        assert T >= m
        u = u[:T - m] + [0] * m
    if mode == TAILBITING:
        reg = [u[(T - d) % T] for d in range(1, m + 1)]     # reg[d-1] = u_{-d}
    else:
        reg = [(start_state >> (d - 1)) & 1 for d in range(1, m + 1)]
    first = list(reg)
    out = []
    for t in range(T):
        x = [u[t]] + reg                                    # x[d] = u_{t-d}
        for j in range(n):
            if keep is None or (keep[t % len(keep)] >> j) & 1:
                out.append(sum(gen[j][0][d] & x[d] for d in range(m + 1)) & 1)
        reg = x[:m]
    if mode == TAILBITING:
        assert reg == first
    return np.array(out, np.uint8)


def span_of(n, T, keep=None):
    if keep is None:
        return n * T
    cnt = [bin(v).count("1") for v in keep]
    return (T // len(cnt)) * sum(cnt) + sum(cnt[:T % len(cnt)])


def encode_ref(gen, n, m, u, T, mode, start_state=0, keep=None, format="bytes", amplitude=0, nout=None, start=0,
               stride=None, offsets=None):
    """The whole output buffer of cvd_encode_frames as bytes (uint8; soft: the int8 values' bytes),
    its length rounded up to 16, and (written, skipped).  u: 0/1 array [F, >= T]."""
    F = len(u)
    span = span_of(n, T, keep)
    if offsets is None:
        stride = span if stride is None else stride
        offs = [start + f * stride for f in range(F)]
    else:
        offs = [int(o) for o in offsets]
    if nout is None:
        nout = max(offs) + span if F else 0
    pos = np.zeros(nout, np.uint8)
    cov = np.zeros(nout, bool)
    written = skipped = 0
    for f in range(F):
        o = offs[f]
        if o < 0 or o + span > nout:
            assert offsets is not None
            skipped += 1
            continue
        pos[o:o + span] = frame_bits(gen, n, m, u[f], T, mode, start_state, keep)
        cov[o:o + span] = True
        written += 1
    fmt = FORMATS[format]
    if fmt == BYTES:
        raw = pos
    elif fmt == SOFT:
        raw = np.where(cov, np.where(pos == 1, amplitude, -amplitude), 0).astype(np.int8).view(np.uint8)
    else:
        raw = np.packbits(pos, bitorder="little" if fmt == LSB else "big")
    buf = np.zeros((len(raw) + 15) // 16 * 16, np.uint8)
    buf[:len(raw)] = raw
    return buf, written, skipped


def golden_pairs():
    """The reference project's own encoder on five codes (tests/golden/parity.npz, */enc_u ->
    */enc_v): (name, gen, m, u [40], v [n, 40 + m])."""
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = np.load(os.path.join(gold, "parity.npz"))
    with open(os.path.join(gold, "parity.json")) as f:
        codes = json.load(f)["codes"]
    return [(name, c["gens"], c["m"], z[name + "/enc_u"], z[name + "/enc_v"]) for name, c in codes.items()
            if name + "/enc_u" in z.files]


# ── shapes the GPU round trips share with the host test that vets them ──

# tail-biting, noiseless: (m, n, T, F, keep); a tail-biting code at small T need not be injective,
# so the GPU test asserts codeword identity; the host test shows that the tests' reference decoder
# gives status 0 and distance 0 on every one of these frames
TB_ROUNDTRIP = [(2, 2, 7, 16, None), (6, 2, 40, 16, None), (6, 3, 40, 16, None), (8, 2, 33, 8, None),
                (6, 2, 4, 16, None), (6, 2, 48, 16, [3, 2, 1])]
TB_SEED = 77
# tail-biting, BSC(0.02): (m, n, T, F); the host test shows that the reference decoder leaves at
# most 10% of these frames without a tail-biting survivor (status 3)
TB_NOISY = [(6, 2, 64, 96), (6, 3, 40, 96)]
NOISY_P = 0.02
NOISY_SEED = 99


def tb_roundtrip_data(i):
    m, n, T, F, keep = TB_ROUNDTRIP[i]
    return np.random.default_rng(TB_SEED + i).integers(0, 2, (F, T)).astype(np.uint8)


def noisy_frames(gen, n, m, T, F, mode, seed, p=NOISY_P):
    """(u [F, T], sent bits [F, n T], received bits [F, n T]) of random frames through a BSC(p);
    terminated frames carry m zero tail bits."""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2, (F, T)).astype(np.uint8)
    if mode == TERMINATED:
        u[:, T - m:] = 0
    sent = np.stack([frame_bits(gen, n, m, u[f], T, mode) for f in range(F)])
    flips = (rng.random(sent.shape) < p).astype(np.uint8)
    return u, sent, sent ^ flips


# terminated and open frames and the stream, noiseless: (m, n, T, F, keep); the host test shows on
# the tests' reference decoder that the sent bits come back with distance 0
RT_FRAMES = [(2, 2, 40, 8, None), (6, 2, 64, 8, None), (6, 3, 50, 8, None), (8, 2, 70, 4, None), (8, 3, 33, 4, None),
             (6, 2, 60, 8, [3, 2, 1]), (6, 2, 61, 8, [3, 2, 2, 2, 1, 2, 1])]
RT_SEED = 55
# the stream (neither state told to the decoder): the shapes of RT_FRAMES it is sent through; at rate
# 7/8 a stream of 61 steps has more unknowns than it pins down
RT_STREAMS = [1, 2, 5]


def rt_data(i, mode):
    """(u [F, T], start state) of RT_FRAMES[i]: terminated frames carry m zero tail bits from state
    0, open frames and the stream (F = 1 of it) start in a random state."""
    m, n, T, F, keep = RT_FRAMES[i]
    rng = np.random.default_rng(RT_SEED + 10 * i + mode)
    u = rng.integers(0, 2, (F, T)).astype(np.uint8)
    if mode == TERMINATED:
        u[:, T - m:] = 0
        return u, 0
    return u, int(rng.integers(1 << m))


def noisy_soft(recv, seed, amplitude=24, erased=0.03):
    """The received bits as int8 values of +-amplitude with a share of erasures (zeros)."""
    rng = np.random.default_rng(seed)
    soft = (amplitude * (2 * recv.astype(np.int8) - 1)).astype(np.int8)
    soft[rng.random(soft.shape) < erased] = 0
    return soft

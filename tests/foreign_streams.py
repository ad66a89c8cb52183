"""Received words that the model's own generator never makes, for the m = 6 detector's
tests against oracle.c_oracle.Model.score_words: what Detector.scan meets in a capture
(another symbol phase, another code, random bits, constants, a cleaner or noisier channel,
a splice, a burst) beside the model's own H1 / H2 streams.  Host only: numpy and the C
oracle's stream generator."""
import numpy as np

from oracle import c_oracle as C

SEED = 12345
M = 6
KINDS = ["h1", "h2", "clean", "noisy3x", "zeros", "ones", "alt", "random", "phase1", "splice", "burst",
         "inverted", "othercode"]
OTHER = (0o135, 0o163)


def gens(octal_pair):
    """(g1, g2) octal, MSB = the current input -> generator_matrix [n][k][m + 1] (m = 6)."""
    return [[[(g >> (M - d)) & 1 for d in range(M + 1)]] for g in octal_pair]


def code(octal_pair):
    return C.Code(gens(octal_pair), M, 1, 2)


def serial_bits(words):
    """received words [..., N] -> serial bits [..., 2N] (bit 2t + j = output j of step t)."""
    w = np.asarray(words, np.int64)
    return ((w[..., None] >> np.arange(2)) & 1).reshape(w.shape[:-1] + (-1,)).astype(np.uint8)


def words_of_bits(bits):
    """serial bits [..., 2N] -> received words [..., N]."""
    b = np.asarray(bits, np.int64)
    return b[..., 0::2] | (b[..., 1::2] << 1)


def one_stream(kind, dec, p, N, q, cuts=(300, 500), burst=(200, 40)):
    """Sequence q of `kind` for the decoder `dec` (octal pair) at crossover probability p:
    int64 [N].  gen1 is the decoder's own code, gen2 the same code with its outputs swapped;
    the oracle's streams take sequence id q (the second stream of phase1: 1000 + q), the
    numpy generator the seed (SEED, q)."""
    tag = C.lib().oc_grid_tag(N, p)
    g1, g2 = code(dec), code(dec[::-1])
    rng = np.random.default_rng([SEED, q])

    def own(c=g1, pp=p, sid=q):
        return C.stream(c, N, pp, SEED, tag, sid)

    if kind == "h1":
        return own()
    if kind == "h2":
        return own(g2)
    if kind == "clean":
        return own(pp=0.0)
    if kind == "noisy3x":
        return own(pp=min(3 * p, 0.5))
    if kind in ("zeros", "ones", "alt"):
        return np.full(N, {"zeros": 0, "ones": 3, "alt": 1}[kind], np.int64)
    if kind == "random":
        return rng.integers(0, 4, N).astype(np.int64)
    if kind == "phase1":
        bits = np.concatenate([serial_bits(own()), serial_bits(own(sid=1000 + q))])
        return words_of_bits(bits[1:1 + 2 * N])
    if kind == "splice":
        a, b = own(), own(g2)
        return np.concatenate([a[:cuts[0]], b[cuts[0]:cuts[1]], a[cuts[1]:]])
    if kind == "burst":
        a = own()
        a[burst[0]:burst[0] + burst[1]] = rng.integers(0, 4, burst[1])
        return a
    if kind == "inverted":
        return own() ^ 3
    if kind == "othercode":
        return own(code(OTHER))
    raise ValueError(kind)


def kind_minor_words(dec, p, N, replicas, **kw):
    """[len(KINDS) * replicas, N] int32: sequence q has kind q % len(KINDS)."""
    nseq = len(KINDS) * replicas
    return np.stack([one_stream(KINDS[q % len(KINDS)], dec, p, N, q, **kw) for q in range(nseq)]).astype(np.int32)


def pack_layout(words):
    """received words [nseq, N] (n = 2) -> uint32 [W/4, nseq, 4], the stream buffer's layout
    (include/cvd.h): word w = steps [16w, 16w + 16), step t at bits 2 (t % 16); W = whole
    16-byte chunks, zero padded."""
    w = np.asarray(words, np.uint64)
    nseq, N = w.shape
    W = ((N + 15) // 16 + 3) // 4 * 4
    pad = np.zeros((nseq, W * 16), np.uint64)
    pad[:, :N] = w
    packed = (pad.reshape(nseq, W, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=2).astype(np.uint32)
    return np.ascontiguousarray(packed.reshape(nseq, W // 4, 4).transpose(1, 0, 2))


# ───────────── the models and shape of test_gpu_foreign_streams.py ─────────────

N, REPL, LEARN = 773, 12, 300_000
NK = len(KINDS)
NSEQ = NK * REPL
MAIN = (0o133, 0o171)
MODELS = [(MAIN, 0.01), (MAIN, 0.05), (MAIN, 0.2), ((0o171, 0o133), 0.05), ((0o135, 0o163), 0.05),
          ((0o133, 0o65), 0.05), ((0o133, 0o133), 0.05)]
IDS = ["%o_%o_p%g" % (d[0], d[1], p) for d, p in MODELS]
MID_STREAM_C2 = {"133_171_p0.01": 1, "135_163_p0.05": 1}   # steps with c > 1 at t > 0 (the oracle)


def reference(dec, p):
    """(oracle model, words [NSEQ, N], sums [NSEQ, 2], stats [NSEQ, 4]) of one decoder / p;
    the arrays are read-only.  g1 = g2 enumerates (one state), so enum_cap = 0 there forces
    the sparse model."""
    om = C.Model(code(dec), p, LEARN, 200, 1.0, SEED, enum_cap=0 if dec[0] == dec[1] else 500_000)
    words = kind_minor_words(dec, p, N, REPL)
    want, stats = om.score_words(words)
    for a in (words, want, stats):
        a.setflags(write=False)
    return om, words, want, stats


def check_inputs(mid, dec, p, stats):
    """The conditions on the inputs, on the oracle's stats alone (the measured values:
    test_gpu_foreign_streams.py's docstring)."""
    tot = stats.reshape(REPL, NK, 4).sum(axis=0)
    share = dict(zip(KINDS, tot[:, 0] / (REPL * N)))
    reent = dict(zip(KINDS, tot[:, 1]))
    if dec[0] == dec[1]:
        assert (stats[:, 2] == N).all(), mid
        return
    assert (stats[:, 2] - stats[:, 3] == 1).all(), mid                  # step 0: c = 2, every sequence
    assert stats[:, 3].sum() == MID_STREAM_C2.get(mid, 0) <= 2, (mid, stats[:, 3].sum())
    if p == 0.2:
        assert max(share.values()) <= 0.05, (mid, share)                 # the all-miss regime
        return
    codeword, foreign = ("alt", "ones") if dec == (0o133, 0o65) else ("ones", "alt")
    for kind in ("clean", "zeros", codeword):
        assert share[kind] >= 0.9, (mid, kind, share[kind])
    for kind in ("random", "phase1", foreign):
        assert share[kind] <= 0.05, (mid, kind, share[kind])
    assert reent["noisy3x"] >= 60, (mid, reent)
    assert reent["burst"] >= 24 and reent["splice"] >= 24, (mid, reent)

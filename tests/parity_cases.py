"""Templates, window lengths and buffers for the parity-template detector's shape tests,
shared by test_parity_cases_host.py (CPU: the conditions on these inputs) and
test_gpu_parity_template_shapes.py (GPU: cvd_parity_detect against the oracle's count on
them).  Host only: numpy and oracle.parity.

cvd_parity_detect compiles one kernel per (n, T0, T1) for n <= 2 -- T0 in {4, 8, 16, 32} the
padded number of terms read from the (current, previous) word pair, T1 in {0, 32} whether any
term is read from the (previous, one before) pair -- and one kernel with 64-bit windows for
n = 3.  group_counts restates from include/cvd.h which group a term falls in, TEMPLATES holds
one template per kernel instance and per n = 3 window edge, and N_VALUES the window lengths
around the 16-byte chunks (4 words) the kernel streams and masks at their edges."""
import numpy as np

NSEQ = 321      # two blocks of 256, the last wave holding one lane
N_H1 = 150      # the H1 / H2 border inside a wave


def spw_of(n):
    """Steps per 32-bit word."""
    return 32 // n


# ─────────────────────────────── term groups ────────────────────────────────

def offset(n, term):
    """o = n*s - j: stream bits from the term's bit back to its anchor's bit (include/cvd.h)."""
    j, s = term
    return n * s - j


def term_at(n, o):
    """The term (j, s) of n <= 2 that lies o stream bits behind its anchor's bit."""
    j = (-o) % n
    return (j, (o + j) // n)


def group_counts(n, template):
    """include/cvd.h, cvd_parity_detect.  n <= 2: (terms with 1 <= o <= 32, terms with
    33 <= o <= 64, terms with o <= 0, T0, T1) with T0 the first of 4, 8, 16, 32 that holds the
    first count and T1 = 32 if the second group has a term, else 0.  n = 3: the number of
    terms per output."""
    if n == 3:
        return tuple(sum(1 for (j, _) in template if j == out) for out in range(3))
    o = [offset(n, t) for t in template]
    assert all(x <= 64 for x in o)
    c0 = sum(1 for x in o if 1 <= x <= 32)
    c1 = sum(1 for x in o if 33 <= x <= 64)
    cz = sum(1 for x in o if x <= 0)
    T0 = next(b for b in (4, 8, 16, 32) if c0 <= b)
    return c0, c1, cz, T0, 32 if c1 else 0


def first_of(template):
    """The first anchor: the template's largest delay."""
    return max(s for (_, s) in template)


# ──────────────────────────────── templates ─────────────────────────────────

G0_EDGES, G1_EDGES = (1, 31, 32), (33, 63, 64)
ZERO_EDGES = {1: (0,), 2: (0, -1)}
# offsets per (T0, T1) instance, the same for n = 1 and n = 2 apart from o = -1, which only
# n = 2 has (the term (1, 0)); every populated group holds its boundary offsets
_G0 = {5: (1, 7, 16, 31, 32), 8: (1, 2, 3, 5, 8, 13, 31, 32), 9: (1, 4, 9, 10, 17, 24, 30, 31, 32),
       16: (1, 2, 3, 4, 6, 9, 11, 14, 15, 16, 20, 25, 29, 30, 31, 32)}
_OFFSETS = {
    (4, 0): lambda z: z,                                   # zero-offset terms only: first = 0
    (4, 32): lambda z: (33, 50, 63, 64),                   # nothing in the (cur, prev) pair
    (8, 0): lambda z: z + _G0[5],
    (8, 32): lambda z: z + _G0[8] + (33, 41, 63, 64),      # T0 = 8 without a padding slot
    (16, 0): lambda z: z + _G0[9],                         # one term past the T0 = 8 bucket
    (16, 32): lambda z: z + _G0[16] + (33, 34, 47, 62, 63, 64),
    (32, 0): lambda z: z + tuple(range(1, 33)),            # every distinct term with o <= 32
    (32, 32): lambda z: z + tuple(range(1, 65)),           # every distinct term
}
N3_DELAYS = (0, 9, 10, 11, 19, 20, 21, 44, 53, 54)
TEMPLATES = {n: [[term_at(n, o) for o in f(ZERO_EDGES[n])] for f in _OFFSETS.values()] for n in (1, 2)}
TEMPLATES[3] = [
    [(0, 0), (1, 0), (2, 1), (0, 3), (1, 7), (2, 5)],                   # first <= 7: today's shape
    [(0, 0), (2, 0)],                                                   # first = 0, no term on output 1
    [(0, 0), (0, 9), (0, 10), (2, 11), (2, 19)],                        # the previous word's edge (s = 9..11)
    [(0, s) for s in range(32)] + [(1, 20), (2, 21)],                   # 32 terms on one output
    [(0, 44), (1, 9), (2, 10), (1, 0)],                                 # first = 44: head = 2
    [(0, 0), (1, 44), (2, 53), (0, 54), (1, 21), (2, 20), (1, 54)],     # the window's last bit, s = 54
]
INSTANCE_KEYS = list(_OFFSETS)

# one template per n with terms in every group (every output for n = 3), for the launch
# shapes; n <= 2: three terms in the (cur, prev) pair, the T0 = 4 instance with T1 = 32
ALL_GROUPS = {
    1: [term_at(1, o) for o in (0, 1, 31, 32, 33, 64)],
    2: [term_at(2, o) for o in (0, -1, 1, 31, 32, 33, 64)],
    3: [(0, 0), (1, 9), (2, 11), (0, 21), (1, 44), (2, 54)],
}


# ───────────────────────────── window lengths ───────────────────────────────

def N_VALUES(n, first):
    """Window lengths around the kernel's chunk edges: one to six chunks of CS = 4 SPW steps
    (every fill state of a three-chunk prefetch), ends on a chunk, on a word and inside a
    word, and N at and below the first anchor."""
    spw = spw_of(n)
    cs = 4 * spw
    vals = [0, 1, first, first + 1, spw, cs - 1, cs, cs + 1, 2 * cs, 3 * cs - 1, 3 * cs + 1, 4 * cs + spw + 1,
            5 * cs + 3]
    return sorted({v for v in vals if v >= 0})


# ───────────────────────────────── buffers ──────────────────────────────────

def random_words(rng, nseq, N, n):
    """Received words [nseq, N], uniform over the 2^n values."""
    return rng.integers(0, 1 << n, (nseq, N)).astype(np.int64)


def foreign_buffer(rng, words, n):
    """Received words [nseq, N] -> int32 [W/4, nseq, 4] in include/cvd.h's layout, W =
    4 ceil(ceil(N / SPW) / 4) (at least one chunk), with every bit the detector must not
    count random instead of zero: the steps at or past N of the last word, the padding words
    of the last chunk, and bits 30-31 of every n = 3 word."""
    w = np.asarray(words, np.uint64)
    nseq, N = w.shape
    spw = spw_of(n)
    W = max(4, ((N + spw - 1) // spw + 3) // 4 * 4)
    steps = np.zeros((nseq, W * spw), np.uint64)
    steps[:, :N] = w
    shifts = (n * np.arange(spw)).astype(np.uint64)
    packed = (steps.reshape(nseq, W, spw) << shifts).sum(axis=2, dtype=np.uint64)
    live = np.zeros(W * spw, np.uint64)
    live[:N] = (1 << n) - 1
    keep = (live.reshape(W, spw) << shifts).sum(axis=1, dtype=np.uint64)        # [W]: the bits of steps < N
    junk = rng.integers(0, 1 << 32, (nseq, W), dtype=np.uint64)
    out = ((packed & keep) | (junk & ~keep & np.uint64(0xFFFFFFFF))).astype(np.uint32)
    return np.ascontiguousarray(out.reshape(nseq, W // 4, 4).transpose(1, 0, 2)).view(np.int32)


def sat_counts(words, n, template):
    """oracle.parity.satisfied_count's count for every sequence of words [nseq, N] at once:
    int64 [nseq], the anchors t in [first, N) with XOR_{(j, s)} y_j[t - s] = 0."""
    w = np.asarray(words, np.int64)
    nseq, N = w.shape
    first = first_of(template)
    if N <= first:
        return np.zeros(nseq, np.int64)
    y = ((w[:, None, :] >> np.arange(n)[None, :, None]) & 1).astype(np.uint8)   # [nseq, n, N]
    x = np.zeros((nseq, N - first), np.uint8)
    for (j, s) in template:
        x ^= y[:, j, first - s:N - s]
    return (x == 0).sum(axis=1).astype(np.int64)


def fractions(sat, N, first):
    """P̂ per sequence, the detector's own double division; 0.0 without anchors."""
    total = N - first if N > first else 0
    return sat / total if total > 0 else np.zeros(len(sat))


def case_rng(n, index, N):
    return np.random.default_rng([n, index, N])

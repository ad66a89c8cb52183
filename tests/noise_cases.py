"""Crafted thresholds for the bit-sliced BSC noise (spec: oracle/philox.py), built on the
oracle alone.  TEST INFRASTRUCTURE ONLY.

A code bit flips iff its 32-bit uniform u is below thr = floor(p 2^32); implementations compare
the 32 bit-planes with thr most significant first and stop once the bit is decided, so a bit
reaches plane d only if u and thr agree on their top d - 1 bits (chance 2^-(d-1), whatever p).
cvd_generate takes the stream tag and p separately and every 32-bit thr is p = thr / 2^32
exactly, so for a chosen word bit the threshold can be put anywhere relative to its uniform:

* crafted(u, d): thr = u with the plane-d bit toggled -- the bit is decided exactly at plane d
  and flips iff u's plane-d bit is 0; the bits below plane d are u's own or their complement
  (they must not matter);
* crafted_equal(u): thr = u, undecided through plane 32, u < thr false: no flip;
* crafted_above(u): thr = u + 1: flip (decided at the lowest plane where u + 1 differs).

Plane d (1..32) is bit 32 - d of u and thr.  Depth 33 = equal through all 32 planes.

test_noise_cases_host.py checks the helper and the conditions on TARGETS that
test_gpu_noise_depths.py relies on; test_noise_host.py feeds the same cases to the product's
host noise_word."""
import numpy as np

from oracle import philox

MASK32 = 0xFFFFFFFF

# ── the generator launches of test_gpu_noise_depths.py ──────────────────────
SEED = 0x5EED_0BAD_C0DE          # both key words non-zero
TAG = 0x2B1D_5EA7                # a fixed tag (no grid_tag(N, p): thr moves, the uniforms stay)
COUNT, BASE, STRIDE = 130, 11, 3  # two full waves and a 2-lane partial one
BASE_HI = 2 ** 33 + 7            # ctr_hi != 0
N_SHORT = {2: 133, 3: 85}        # 9 received words: two full 4-word chunks + one live word
N_LONG = 4099                    # n = 2: 257 words, 65 chunks -> gridDim.y = 4 segments (enc.seek)

# (sequence index q, word w, word bit b) -> seq_id = base + STRIDE q.  Lanes 0 and 63 of a full
# wave and both lanes of the partial one; w % 4 = 0..3; word 8, the single live word of the last
# chunk (N_SHORT: 5 steps, 10 valid bits for n = 2, 15 for n = 3); bits 0 and 31 (29 for n = 3).
# Over each list, u's bit takes both values at every plane (test_noise_cases_host.py), so both
# outcomes of crafted(u, d) are seen at every depth.
TARGETS = {
    2: [(0, 0, 0), (63, 1, 31), (64, 2, 13), (127, 3, 31), (128, 8, 0), (129, 8, 9), (1, 5, 22), (65, 6, 7)],
    3: [(0, 0, 0), (63, 1, 29), (64, 2, 13), (127, 3, 29), (128, 8, 0), (129, 8, 14), (1, 5, 22), (65, 6, 7)],
}
TARGET_HI = (129, 8, 3)          # the BASE_HI launch (n = 2 and 3)
TARGET_LONG = (63, 256, 1)       # the N_LONG launch: word 256, the live word of the last chunk

DEEP_DEPTHS = (9, 16, 17, 24, 25, 28, 29, 32)   # first and last plane of every straggler block pair

# threshold edges (3c): thr = 0, 1, 2, 2^23, 2^24 - 1, 2^24, 2^30 + 1, 2^31 - 1, 2^31,
# 2^32 - 1 (twice: the second by rounding down) and 2^32
EDGE_P = [0.0, 2.0 ** -32, 2.0 ** -31, 2.0 ** -9, 2.0 ** -8 - 2.0 ** -32, 2.0 ** -8, 0.25 + 2.0 ** -32,
          0.5 - 2.0 ** -32, 0.5, 1 - 2.0 ** -32, float(np.nextafter(1.0, 0.0)), 1.0]
EDGE_THR = [0, 1, 2, 2 ** 23, 2 ** 24 - 1, 2 ** 24, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 1,
            2 ** 32]


def seq_of(q, base=BASE):
    return base + STRIDE * q


def uniform_of(seed, tag, seq_id, w, b):
    """The 32-bit uniform u of word bit b of received word w."""
    return int(philox.noise_word_uniforms(seed, tag, seq_id, [w], 1)[0, b])


def crafted(u, d, complement=False):
    """(thr, flips): thr agrees with u above plane d, differs at plane d; below it u's own bits
    or (complement) their complement."""
    assert 1 <= d <= 32 and 0 <= u <= MASK32
    bit = 1 << (32 - d)
    low = bit - 1
    thr = (u ^ bit) & ~low & MASK32
    thr |= (~u if complement else u) & low
    return thr, int(not u & bit)


def crafted_equal(u):
    return u, 0


def crafted_above(u):
    assert u < MASK32
    return u + 1, 1


def p_of(thr):
    p = thr / 2 ** 32
    assert philox.threshold(p) == thr
    return p


def depth_of(u, thr):
    """First plane (1..32) at which u and thr differ; 33 if none."""
    x = (u ^ thr) & MASK32
    return 33 if x == 0 else 33 - x.bit_length()


def all_cases(u):
    """Every crafted case of one uniform: (label, thr, flips)."""
    out = []
    for d in range(1, 33):
        for comp in (False, True):
            thr, f = crafted(u, d, comp)
            out.append((f"d{d}{'c' if comp else 'o'}", thr, f))
    out.append(("equal",) + crafted_equal(u))
    if u < MASK32:
        out.append(("above",) + crafted_above(u))
    return out


def deep_cases(u):
    """The straggler rounds' cases (3b): DEEP_DEPTHS in u's own filling, and equality."""
    return [(f"d{d}o",) + crafted(u, d) for d in DEEP_DEPTHS] + [("equal",) + crafted_equal(u)]


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _popcount(x):
    return int(_POP8[np.ascontiguousarray(x, dtype=np.uint32).view(np.uint8)].sum())


def depth_histogram(seed, tag, seq_ids, nwords, n, thr, deep_from=None, block=1 << 19):
    """hist[d], d = 1..33 (hist[0] = 0): the number of valid bits (the low (32 // n) n bits of
    words 0..nwords-1 of the sequences `seq_ids`) decided at plane d, 33 = never (u == thr).
    Block by block of four planes on the words that still hold an undecided bit, so the cost is
    that of the first two blocks.  deep_from: also return [(seq_id, w, b, depth)] of the bits
    with depth >= deep_from."""
    assert 0 <= thr <= MASK32
    spw = 32 // n
    valid = np.uint32((1 << (spw * n)) - 1 if spw * n < 32 else MASK32)
    seq_ids = np.asarray(seq_ids, dtype=np.uint64)
    hist = np.zeros(34, np.int64)
    deep = []
    k0, k1 = seed & MASK32, seed >> 32
    per = max(1, block // nwords)
    for s0 in range(0, len(seq_ids), per):
        sid = np.repeat(seq_ids[s0:s0 + per], nwords)
        w = np.tile(np.arange(nwords, dtype=np.uint64), len(sid) // nwords)
        hi = ((sid >> np.uint64(32)) & np.uint64(0xFFFF)) | np.uint64(philox.KIND_NOISE << 16)
        U = np.full(len(sid), valid, np.uint32)
        for j in range(8):
            live = np.nonzero(U)[0]
            if len(live) == 0:
                break
            x = philox.philox4x32_10(w[live] * np.uint64(8) + np.uint64(j), sid[live] & np.uint64(MASK32),
                                     hi[live], np.full(len(live), tag, np.uint64), k0, k1)
            Ul = U[live]
            for i in range(4):
                d = 4 * j + i + 1
                diff = x[i] ^ np.uint32(MASK32 if (thr >> (32 - d)) & 1 else 0)   # u's bit != thr's bit
                dec = Ul & diff
                hist[d] += _popcount(dec)
                if deep_from is not None and d >= deep_from:
                    for r in np.nonzero(dec)[0]:
                        deep += [(int(sid[live[r]]), int(w[live[r]]), b, d) for b in range(32) if (int(dec[r]) >> b) & 1]
                Ul = Ul & ~diff
            U[live] = Ul
        hist[33] += _popcount(U)
        if deep_from is not None:
            for r in np.nonzero(U)[0]:
                deep += [(int(sid[r]), int(w[r]), b, 33) for b in range(32) if (int(U[r]) >> b) & 1]
    return (hist, deep) if deep_from is not None else hist


# ── 3d: the fused kernel's deep planes, found by search (its tag is grid_tag(N, p)) ──
# In the `trials` trials from trial_begin, depth_histogram reports at least three bits decided at
# depth >= 25, in an H1 (even seq_id) and in an H2 sequence; test_gpu_noise_depths.py asserts it.
FUSED_DEEP = {
    "m2": dict(N=1024, p=0.05, seed=20250, trial_begin=1_000_000, trials=32768),
    "r23_m4": dict(N=1000, p=0.05, seed=20250, trial_begin=1_000_000, trials=22370),
}

# ── 3e: the learning chain (LEARN_TAG, sequence 0, n = 2) ──
LEARN_SEED, LEARN_LEN = 12345, 60_000


def learn_target(lo=0.01, hi=0.2, first_word=13):
    """(w, b, u): the first bit past the burn-in (word 13 = step 208) of the learning stream whose
    uniform lies in [lo, hi] 2^32 with room for u + 1 and u - 1."""
    for w in range(first_word, LEARN_LEN // 16):
        us = philox.noise_word_uniforms(LEARN_SEED, philox.LEARN_TAG, 0, [w], 2)[0]
        for b in range(32):
            u = int(us[b])
            if lo * 2 ** 32 + 2 <= u <= hi * 2 ** 32 - 2:
                return w, b, u
    raise AssertionError("no learning target")

"""Cases of the capture front end (csrc/cvd_sweep.hip: cvd_parity_sweep; csrc/cvd_capture.hip:
cvd_pack_windows) and the references of the sweep, in numpy alone.  TEST INFRASTRUCTURE ONLY.

* sweep_reference: the [n_phase, 2^B] array of include/cvd.h from B shifted slices of the bits,
  np.bincount and an int64 Walsh-Hadamard transform: fast enough for millions of anchors.
* sweep_definition: the same array from the definition, sat[f][mask] = #{anchors whose masked
  word has even parity}, one mask at a time, with no word, histogram or transform (B <= 10).
* instance_of / tiles_and_grid: the dispatch rule of cvd_parity_sweep and the launch shape of its
  histogram kernel, restated from the constants in the header comment of csrc/cvd_sweep.hip.
* The case tables: INSTANCE_CASES (all 27 sweep_hist_kernel<n, format, mode>), WHT_CASES (B =
  1..22), STRIDE_CASES (blocks that take a second and a third tile), ALIGN_CASES (starts and ends
  on piece and tile edges), TINY_CASES (T = 1, 2), STRUCTURED_CASES (two bins hold everything),
  the constant capture of 2^31 - 1 anchors, and the PACK_* tables of cvd_pack_windows.

test_sweep_cases_host.py proves the references against each other and every property the tables
were chosen for; test_gpu_sweep_edges.py runs the tables through the kernels."""
import zlib
from collections import namedtuple

import numpy as np

FORMATS = ("lsb", "msb", "bytes")
MODES = ("whole", "parts", "global")

# csrc/cvd_sweep.hip, header comment
PIECE_BITS = 128                     # a 16-byte piece of a packed capture
TILE_PIECES = 512
TILE_BITS = TILE_PIECES * PIECE_BITS  # 65,536 capture bits per tile
LDS_MAX_B = 15                       # largest B with the whole histogram in LDS
GLOBAL_MIN_B = 22                    # smallest B on global atomics (CVD_SWEEP_GLOBAL_B moves it, floor 16)
MAX_B = 22
MAX_GRID_X = 1024

# a sweep: bits `fill` ("random", "ones", "alt" = 0101...), global_b = CVD_SWEEP_GLOBAL_B or None,
# pad: the capture may end on a piece, so a further piece of ones is allocated behind it
Sweep = namedtuple("Sweep", "n span start T n_phase fmt global_b fill pad", defaults=(None, "random", False))


def sweep_id(c):
    tail = ("" if c.global_b is None else f"_g{c.global_b}") + ("" if c.fill == "random" else "_" + c.fill)
    return f"n{c.n}_s{c.span}_st{c.start}_T{c.T}_f{c.n_phase}_{c.fmt}{tail}"


def word_bits(c):
    return c.n * (c.span + 1)


def last_first(c):
    """first capture bit of the last word of the last phase"""
    return c.start + (c.n_phase - 1) + c.n * (c.T - 1)


def sweep_nbits(c):
    """the last word ends on the capture's last bit"""
    return last_first(c) + word_bits(c)


def _seed(c):
    return zlib.crc32(repr(tuple(c)).encode())


def make_bits(fill, nbits, seed):
    if fill == "ones":
        return np.ones(nbits, np.uint8)
    if fill == "zeros":
        return np.zeros(nbits, np.uint8)
    if fill == "alt":
        return (np.arange(nbits) & 1).astype(np.uint8)
    assert fill == "random"
    return np.random.default_rng(seed).integers(0, 2, nbits).astype(np.uint8)


def case_bits(c):
    return make_bits(c.fill, sweep_nbits(c), _seed(c))


# ───────────────────────────────── references ───────────────────────────────

def wht(v):
    """W[a] = sum_x v[x] (-1)^popcount(a & x), int64, in place on a copy."""
    v = np.array(v, np.int64)
    h = 1
    while h < len(v):
        p = v.reshape(-1, 2, h)
        lo = p[:, 0, :].copy()
        p[:, 0, :] += p[:, 1, :]
        np.subtract(lo, p[:, 1, :], out=p[:, 1, :])
        h *= 2
    return v


def words_of(bits, n, span, first, T):
    """word a = sum_b bits[first + n a + b] << b, from B strided slices"""
    B = n * (span + 1)
    assert T >= 1 and first >= 0 and first + n * (T - 1) + B <= len(bits)
    word = np.zeros(T, np.uint32)
    for b in range(B):
        word |= bits[first + b:first + b + n * (T - 1) + 1:n].astype(np.uint32) << np.uint32(b)
    return word


def sweep_reference(bits, n, span, start, T, n_phase):
    """cvd_parity_sweep into a zeroed d_sat, as include/cvd.h states it: int64 [n_phase, 2^B]."""
    B = n * (span + 1)
    out = np.zeros((n_phase, 1 << B), np.int64)
    for f in range(n_phase):
        hist = np.bincount(words_of(bits, n, span, start + f, T), minlength=1 << B)
        out[f] = (T + wht(hist)) // 2
    return out


def sweep_definition(bits, n, span, start, T, n_phase):
    """sat[f][mask] = #{a < T : the bits start + f + n a + b, b in mask, have an even sum}."""
    B = n * (span + 1)
    assert B <= 10
    out = np.zeros((n_phase, 1 << B), np.int64)
    for f in range(n_phase):
        first = start + f
        assert first + n * (T - 1) + B <= len(bits)
        column = [bits[first + b:first + b + n * (T - 1) + 1:n] for b in range(B)]
        for mask in range(1 << B):
            odd = np.zeros(T, np.uint8)
            for b in range(B):
                if (mask >> b) & 1:
                    odd ^= column[b]
            out[f, mask] = T - int(odd.sum(dtype=np.int64))
    return out


def case_reference(c, bits=None):
    bits = case_bits(c) if bits is None else bits
    return sweep_reference(bits, c.n, c.span, c.start, c.T, c.n_phase)


def constant_sat(value, B, T, n_phase):
    """The sweep of a constant capture in closed form.  All zeros: every word is 0 and satisfies
    every mask.  All ones: every word is 2^B - 1, and popcount(word & mask) = popcount(mask)."""
    if value == 0:
        return np.full((n_phase, 1 << B), T, np.int64)
    m = np.arange(1 << B, dtype=np.int64)
    weight = np.zeros(1 << B, np.int64)
    for b in range(B):
        weight += (m >> b) & 1
    return np.broadcast_to(np.where(weight % 2 == 0, T, 0), (n_phase, 1 << B)).astype(np.int64)


# ─────────────────────────── dispatch and launch shape ──────────────────────

def instance_of(n, span, fmt, global_b=None):
    """(mode, n, format) of the sweep_hist_kernel that cvd_parity_sweep launches."""
    B = n * (span + 1)
    assert 1 <= n <= 3 and 1 <= B <= MAX_B and fmt in FORMATS
    gb = GLOBAL_MIN_B if global_b is None else max(LDS_MAX_B + 1, int(global_b))
    mode = "whole" if B <= LDS_MAX_B else "global" if B >= gb else "parts"
    return mode, n, fmt


def tiles_and_grid(n, span, start, T, n_phase, global_b=None):
    """(ntiles, gridDim.x) of the histogram launch: tile 0 begins at the piece of `start`."""
    B = n * (span + 1)
    mode = instance_of(n, span, "lsb", global_b)[0]
    parts = 1 << (B - LDS_MAX_B) if mode == "parts" else 1
    g0 = start >> 7
    glast = (start + (n_phase - 1) + n * (T - 1)) >> 7
    ntiles = (glast - g0) // TILE_PIECES + 1
    return ntiles, min(ntiles, max(1, MAX_GRID_X // (n_phase * parts)))


def case_grid(c):
    return tiles_and_grid(c.n, c.span, c.start, c.T, c.n_phase, c.global_b)


# ───────────────────────────── every instance, every B ──────────────────────

# span per (mode, n), one per format in FORMATS' order; n_phase = n, 2,000 <= T <= 6,000, odd start
_INSTANCE_SPANS = {
    ("whole", 1): (10, 12, 14),      # B = 11, 13, 15
    ("whole", 2): (4, 5, 6),         # B = 10, 12, 14
    ("whole", 3): (2, 3, 4),         # B = 9, 12, 15
    ("parts", 1): (15, 16, 18),      # B = 16, 17, 19
    ("parts", 2): (7, 8, 9),         # B = 16, 18, 20
    ("parts", 3): (5, 6, 5),         # B = 18, 21, 18
    ("global", 1): (21, 21, 21),     # B = 22, natively
    ("global", 2): (10, 10, 10),     # B = 22, natively
    ("global", 3): (5, 5, 5),        # B = 18: n = 3 has no B = 22; CVD_SWEEP_GLOBAL_B = 16
}
ENV_GLOBAL_B = 16


def _instance_cases():
    out = []
    for i, ((mode, n), spans) in enumerate(sorted(_INSTANCE_SPANS.items())):
        for j, fmt in enumerate(FORMATS):
            gb = ENV_GLOBAL_B if (mode, n) == ("global", 3) else None
            out.append(Sweep(n, spans[j], 2 * (7 * i + 3 * j) + 1, 2003 + 431 * ((3 * i + j) % 10), n, fmt, gb))
    return out


INSTANCE_CASES = _instance_cases()
WHT_CASES = [Sweep(1, B - 1, 5, 3001, 1, FORMATS[B % 3]) for B in range(1, MAX_B + 1)]

# ───────────────────────────────── grid stride ──────────────────────────────

# case, (ntiles, gx): blocks 0 .. ntiles - gx - 1 take a second tile (and block 0 of the first a third)
STRIDE_CASES = [
    (Sweep(3, 6, 5, 240_000, 3, "lsb"), (11, 5)),           # B = 21: 64 parts; tiles 0, 5, 10 in block 0
    (Sweep(2, 9, 3, 1_080_001, 2, "bytes"), (33, 16)),      # B = 20: 32 parts; two passes and one tile more
    (Sweep(1, 15, 1, 150_001, 1, "msb"), (3, 3)),           # B = 16: the control, one block per tile
    (Sweep(3, 1, 7, 7_490_001, 3, "msb"), (343, 341)),      # B = 6 whole: two blocks keep their LDS histogram
    (Sweep(3, 5, 7, 7_490_001, 3, "lsb", ENV_GLOBAL_B), (343, 341)),   # the same stride on global atomics
]

# ───────────────────────────────── alignment ────────────────────────────────

ALIGN_INSTANCES = [(3, 2, "lsb"), (3, 2, "msb"), (3, 2, "bytes"), (2, 3, "bytes")]   # n, span, format
ALIGN_STARTS = [0, 1, 127, PIECE_BITS * 513 + 127]      # the last: g0 = 513, tile 0 is not the buffer's first piece
ALIGN_ENDS = ["tile_last_bit", "next_tile_first_bit", "piece_end", "tile_end"]


def align_case(n, span, fmt, start, end):
    """The sweep from `start` whose last word begins on a tile's last bit / on the next tile's
    first bit, or whose capture ends on a piece that is no tile edge / on a tile edge (tiles are
    counted from the piece of `start`).  n_phase = n where the residues allow it (n = 3: always,
    since 65,536 = 1 mod 3 and the tile may be chosen; n = 2: for one parity of `start`)."""
    B = n * (span + 1)
    tile0 = (start >> 7) << 7
    for n_phase in range(n, 0, -1):
        for k in (2, 3, 4):
            lf = {"tile_last_bit": tile0 + k * TILE_BITS - 1,
                  "next_tile_first_bit": tile0 + k * TILE_BITS,
                  "piece_end": tile0 + k * TILE_BITS + 5 * PIECE_BITS - B,
                  "tile_end": tile0 + k * TILE_BITS - B}[end]
            d = lf - start - (n_phase - 1)
            if d >= 0 and d % n == 0:
                return Sweep(n, span, start, d // n + 1, n_phase, fmt, pad=end in ("piece_end", "tile_end"))
    raise AssertionError((n, span, start, end))


ALIGN_CASES = [(end, align_case(n, span, fmt, start, end))
               for n, span, fmt in ALIGN_INSTANCES for start in ALIGN_STARTS for end in ALIGN_ENDS]

# T = 1 and 2 at every (n, format); the first word begins on a piece's last bit
TINY_CASES = [Sweep(n, 2, 127, T, n, fmt) for n in (1, 2, 3) for fmt in FORMATS for T in (1, 2)]

# all ones: one bin; 0101...: two bins (n = 1: the words that begin on an even and on an odd bit)
STRUCTURED_CASES = [Sweep(1, B - 1, 3, 4099, 1, FORMATS[i % 2], None, fill)
                    for i, B in enumerate((13, 16, 19, 22)) for fill in ("ones", "alt")]

# the i32 edge: 2^31 - 1 anchors in one bin of an LSB capture made on the device
I32_NBITS = (1 << 31) + 128
I32_CASE = Sweep(1, 3, 0, (1 << 31) - 1, 1, "lsb")

# ───────────────────────────────── window packing ───────────────────────────

# csrc/cvd_capture.hip, header comment
PACK_SEQS = 64                       # sequences per tile
PACK_CHUNKS = 32                     # 16-byte chunks (four layout words) per sequence and tile
PACK_ROW_DWORDS = 4 * (PACK_CHUNKS + 1)

Pack = namedtuple("Pack", "n N start stride nwin n_phase fmt pad", defaults=(False,))


def pack_id(c):
    return f"n{c.n}_N{c.N}_s{c.start}_d{c.stride}_w{c.nwin}_f{c.n_phase}_{c.fmt}"


def pack_nbits(c):
    """the last window of the last phase ends on the capture's last bit"""
    return c.start + (c.nwin - 1) * c.stride + (c.n_phase - 1) + c.N * c.n


def pack_bits(c):
    return make_bits("random", pack_nbits(c), _seed(c))


def steps_per_word(n):
    return 32 // n


def pack_tile_bits(n):
    """capture bits of a full tile of 32 chunks"""
    return 4 * PACK_CHUNKS * steps_per_word(n) * n


def pack_steps(n, extra):
    """N of one full chunk tile and `extra` steps more"""
    return 4 * PACK_CHUNKS * steps_per_word(n) + extra


def pack_offsets(c, ctile):
    """(win_bit + tile_bits) & 127 of every sequence at chunk tile `ctile`: the funnel's offset"""
    q = np.arange(c.nwin * c.n_phase, dtype=np.int64)
    win_bit = c.start + (q // c.n_phase) * c.stride + q % c.n_phase
    return (win_bit + ctile * pack_tile_bits(c.n)) & 127


_PACK_STRIDES = (77, 129, 255, 1001, 4097, 3, 8191, 127, 2049)       # odd: units mod 128
# one per pack_windows_kernel<n, format>: 130 windows (sequence tiles of 64, 64 and 2 rows), every
# funnel offset 0..127, N = 32 chunks + 5 steps (a second chunk tile of one chunk, its word ragged)
PACK_INSTANCE_CASES = [Pack(n, pack_steps(n, 5), 2 * (3 * (n - 1) + j) + 1, _PACK_STRIDES[3 * (n - 1) + j], 130, 1, fmt)
                       for n in (1, 2, 3) for j, fmt in enumerate(FORMATS)]
PACK_Q0, PACK_EXTRA_PITCH = 3, 9

PACK_PHASE_CASES = [Pack(n, pack_steps(n, 5), 9, 131, 70, n, fmt) for n in (2, 3) for fmt in ("bytes", "lsb")]


def _pack_piece_end(n, fmt):
    """the last window ends exactly where a 128-bit piece of the capture ends"""
    c = Pack(n, pack_steps(n, 5), 0, 131, 70, 1, fmt, True)
    return c._replace(start=-pack_nbits(c) % PIECE_BITS)


PACK_PIECE_END_CASES = [_pack_piece_end(n, fmt) for n in (2, 3) for fmt in ("bytes", "lsb")]

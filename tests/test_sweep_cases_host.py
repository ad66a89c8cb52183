"""tests/sweep_cases.py on the CPU: the fast reference of cvd_parity_sweep equals the restatement
of test_gpu_sweep.py at that file's shapes and equals the definition (count the anchors whose
masked word has even parity) where the definition is affordable, so the reference that
test_gpu_sweep_edges.py gives the kernels is the contract of include/cvd.h; and every property
the case tables were chosen for, from the reference and the constants documented in the kernels'
header comments alone: the 27 + 9 instances, B = 1..22, ntiles > gx in the stride cases, the
residues and end alignments of the alignment cases, the funnel offsets of the pack cases."""
import numpy as np
import pytest

import sweep_cases as SC
from test_gpu_sweep import SWEEP_CASES, sweep_restatement     # imports without a device

ALL_SWEEPS = (SC.INSTANCE_CASES + SC.WHT_CASES + [c for c, _ in SC.STRIDE_CASES] + [c for _, c in SC.ALIGN_CASES]
              + SC.TINY_CASES + SC.STRUCTURED_CASES)


# ── the references ──────────────────────────────────────────────────────────

@pytest.mark.parametrize("case", SWEEP_CASES, ids=lambda c: "n{}_s{}_st{}_T{}_f{}_{}".format(*c))
def test_reference_equals_restatement(case):
    assert len(SWEEP_CASES) == 13
    n, span, start, T, n_phase, _ = case
    bits = SC.make_bits("random", start + (n_phase - 1) + n * (T - 1) + n * (span + 1), 17)
    assert np.array_equal(SC.sweep_reference(bits, n, span, start, T, n_phase),
                          sweep_restatement(bits, n, span, start, T, n_phase))


@pytest.mark.parametrize("fill", ["random", "ones", "alt"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_reference_equals_definition(n, fill):
    """every B <= 10 of this n, n_phase = n; T is odd and no multiple of n"""
    for span in range(10 // n):
        B = n * (span + 1)
        start, T = 3 + span, 301 - 2 * span
        bits = SC.make_bits(fill, start + (n - 1) + n * (T - 1) + B + 2, 100 * n + span)
        ref = SC.sweep_reference(bits, n, span, start, T, n)
        assert ref.shape == (n, 1 << B) and ref.dtype == np.int64
        assert np.array_equal(ref, SC.sweep_definition(bits, n, span, start, T, n)), (n, span)
        assert np.all(ref[:, 0] == T)
    assert B >= 9


def test_definition_by_hand():
    """bits 1 1 0 1 0, n = 1, span 1, three anchors: words (b0, b1) = 11, 10, 01"""
    bits = np.array([1, 1, 0, 1, 0], np.uint8)
    # mask 0: all; mask 1 (bit 0): b0 = 0 once; mask 2: b1 = 0 once; mask 3: b0 = b1 once
    assert SC.sweep_definition(bits, 1, 1, 0, 3, 1).tolist() == [[3, 1, 1, 1]]
    assert SC.sweep_reference(bits, 1, 1, 0, 3, 1).tolist() == [[3, 1, 1, 1]]
    # from bit 1: (b0, b1) = 10, 01, 10 -> b0 = 0 once, b1 = 0 twice, equal never
    assert SC.sweep_definition(bits, 1, 1, 1, 3, 1).tolist() == [[3, 1, 2, 0]]
    # two phases of n = 2, span 0, two anchors: phase 0 (b0, b1) = 11, 01; phase 1 = 10, 10
    assert SC.sweep_definition(bits, 2, 0, 0, 2, 2).tolist() == [[2, 1, 0, 1], [2, 0, 2, 0]]
    assert SC.sweep_reference(bits, 2, 0, 0, 2, 2).tolist() == [[2, 1, 0, 1], [2, 0, 2, 0]]


def test_constant_capture_closed_forms():
    """what the test of 2^31 - 1 anchors expects, checked where the reference can be computed"""
    c = SC.I32_CASE
    B, T = SC.word_bits(c), 70_001
    assert (c.n, c.span, c.n_phase, c.fmt, c.start, B) == (1, 3, 1, "lsb", 0, 4)
    for value, fill in ((0, "zeros"), (1, "ones")):
        bits = SC.make_bits(fill, T + c.span, 0)
        assert np.array_equal(SC.constant_sat(value, B, T, 1), SC.sweep_reference(bits, c.n, c.span, 0, T, 1))
    assert SC.constant_sat(1, B, T, 1)[0].tolist() == [T if bin(m).count("1") % 2 == 0 else 0 for m in range(16)]
    # the large case itself: the last word ends inside the capture, and the count is the i32 edge
    assert c.T == 2 ** 31 - 1 and SC.sweep_nbits(c) == 2 ** 31 + 2 <= SC.I32_NBITS
    assert SC.I32_NBITS % 128 == 0 and SC.instance_of(c.n, c.span, c.fmt) == ("whole", 1, "lsb")
    assert SC.case_grid(c) == (2 ** 31 // SC.TILE_BITS, 1024)


# ── dispatch and launch shape ───────────────────────────────────────────────

def test_instance_of_restates_the_dispatch_rule():
    assert SC.instance_of(3, 4, "bytes") == ("whole", 3, "bytes")         # B = 15
    assert SC.instance_of(2, 7, "lsb") == ("parts", 2, "lsb")             # B = 16
    assert SC.instance_of(3, 6, "msb") == ("parts", 3, "msb")             # B = 21
    assert SC.instance_of(1, 21, "lsb") == ("global", 1, "lsb")           # B = 22
    assert SC.instance_of(2, 7, "lsb", 16) == ("global", 2, "lsb")
    assert SC.instance_of(2, 7, "lsb", 3) == ("global", 2, "lsb")         # the floor: 16
    assert SC.instance_of(3, 4, "lsb", 3) == ("whole", 3, "lsb")          # ... so B = 15 stays in LDS
    assert SC.instance_of(2, 10, "lsb", 23) == ("parts", 2, "lsb")
    # n = 3 has no B = 22, and no B = 16
    assert 22 not in {3 * (s + 1) for s in range(8)} and 16 not in {3 * (s + 1) for s in range(8)}


def test_tiles_and_grid_at_the_existing_shapes():
    """the issue's reading of test_gpu_sweep.py: no exact-comparison case there strides"""
    for n, span, start, T, n_phase, _ in SWEEP_CASES:
        ntiles, gx = SC.tiles_and_grid(n, span, start, T, n_phase)
        assert ntiles <= 4 and gx == ntiles
    assert SC.tiles_and_grid(2, 7, 5, 70_001, 2) == (3, 3)
    assert SC.tiles_and_grid(1, 3, 0, 2 ** 31 - 1, 1) == (32768, 1024)    # the 256-MiB test does


def test_instance_table_is_all_27():
    got = [SC.instance_of(c.n, c.span, c.fmt, c.global_b) for c in SC.INSTANCE_CASES]
    assert len(got) == 27 and set(got) == {(m, n, f) for m in SC.MODES for n in (1, 2, 3) for f in SC.FORMATS}
    for c, (mode, _, _) in zip(SC.INSTANCE_CASES, got):
        B = SC.word_bits(c)
        assert c.n_phase == c.n and 2000 <= c.T <= 6000 and c.start % 2 == 1 and c.fill == "random" and not c.pad
        assert {"whole": B <= 15, "parts": 16 <= B <= 21, "global": B >= 16}[mode]
        if mode == "global":
            # natively at B = 22; n = 3 only through the environment, at B = 18
            assert (c.global_b, B) == ((16, 18) if c.n == 3 else (None, 22))
            if c.n == 3:
                assert SC.instance_of(c.n, c.span, c.fmt) == ("parts", 3, c.fmt)
        else:
            assert c.global_b is None
    assert len({SC.sweep_id(c) for c in SC.INSTANCE_CASES}) == 27


def test_wht_table_is_every_B():
    assert [SC.word_bits(c) for c in SC.WHT_CASES] == list(range(1, 23))
    assert all(c.n == 1 and c.T == 3001 and c.n_phase == 1 for c in SC.WHT_CASES)
    assert {c.fmt for c in SC.WHT_CASES} == set(SC.FORMATS)
    assert all(a.fmt != b.fmt for a, b in zip(SC.WHT_CASES, SC.WHT_CASES[1:]))
    # B = 1..7: the transform's block of max(64, 2^B / 2) threads has more threads than butterflies
    assert [B for B in range(1, 23) if max(64, 2 ** B // 2) > 2 ** B // 2] == [1, 2, 3, 4, 5, 6]
    assert 64 >= 2 ** 7 // 2


def test_every_sweep_case_is_a_valid_call():
    ids = set()
    for c in ALL_SWEEPS + [SC.I32_CASE]:
        B = SC.word_bits(c)
        assert 1 <= c.n <= 3 and 1 <= B <= 22 and 1 <= c.n_phase <= c.n and c.start >= 0 and 1 <= c.T < 2 ** 31
        assert SC.sweep_nbits(c) == c.start + (c.n_phase - 1) + c.n * (c.T - 1) + B
        # only the cases that say so end on a piece (they get a piece of ones behind the capture)
        assert c.pad == (SC.sweep_nbits(c) % 128 == 0) or c is SC.I32_CASE
        ids.add(SC.sweep_id(c))
    assert len(ids) == len(ALL_SWEEPS) + 1


# ── grid stride ─────────────────────────────────────────────────────────────

def test_stride_cases_stride():
    want = [("parts", 3, "lsb", 21, (11, 5)), ("parts", 2, "bytes", 20, (33, 16)), ("parts", 1, "msb", 16, (3, 3)),
            ("whole", 3, "msb", 6, (343, 341)), ("global", 3, "lsb", 18, (343, 341))]
    assert len(SC.STRIDE_CASES) == len(want)
    for (c, shape), (mode, n, fmt, B, stated) in zip(SC.STRIDE_CASES, want):
        assert SC.instance_of(c.n, c.span, c.fmt, c.global_b) == (mode, n, fmt) and SC.word_bits(c) == B
        assert c.n_phase == c.n
        assert SC.case_grid(c) == shape == stated
        ntiles, gx = shape
        # the last word begins in the last tile, so that tile is not empty
        assert (SC.last_first(c) - ((c.start >> 7) << 7)) // SC.TILE_BITS == ntiles - 1
        # every tile holds words of every phase
        assert c.start + c.n_phase <= SC.TILE_BITS
    (a, b, ctl, w, g) = [s for _, s in SC.STRIDE_CASES]
    assert a[0] > 2 * a[1] and -(-a[0] // a[1]) == 3          # two passes and a ragged third, in block 0 alone
    assert b[0] == 2 * b[1] + 1                               # two passes everywhere, a third in block 0
    assert ctl[0] == ctl[1]                                   # the control does not stride
    assert w[0] - w[1] == g[0] - g[1] == 2                    # two blocks take a second tile


# ── alignment ───────────────────────────────────────────────────────────────

def test_alignment_cases_have_the_stated_residues():
    assert len(SC.ALIGN_CASES) == 4 * 4 * 4
    assert {(c.n, c.fmt) for _, c in SC.ALIGN_CASES} == {(3, "lsb"), (3, "msb"), (3, "bytes"), (2, "bytes")}
    assert sorted({c.start % 128 for _, c in SC.ALIGN_CASES}) == [0, 1, 127]
    assert max(c.start for _, c in SC.ALIGN_CASES) >= 128 * 512 + 127
    for n, fmt in {(c.n, c.fmt) for _, c in SC.ALIGN_CASES}:
        mine = [(end, c) for end, c in SC.ALIGN_CASES if (c.n, c.fmt) == (n, fmt)]
        assert {(end, c.start) for end, c in mine} == {(e, s) for e in SC.ALIGN_ENDS for s in SC.ALIGN_STARTS}
        if n == 3:
            assert all(c.n_phase == 3 for _, c in mine)
        else:
            assert all(c.n_phase in (1, 2) for _, c in mine) and {c.n_phase for _, c in mine} == {1, 2}
    for end, c in SC.ALIGN_CASES:
        B, g0 = SC.word_bits(c), c.start >> 7
        tile0 = g0 * 128                                      # capture bit of tile 0's first bit
        lf, nbits = SC.last_first(c), SC.sweep_nbits(c)
        ntiles, gx = SC.case_grid(c)
        assert 2 <= ntiles <= 5 and gx == ntiles and SC.instance_of(c.n, c.span, c.fmt)[0] == "whole"
        pieces = -(-nbits // 128)                             # the capture's 128-bit pieces (nu4, packed)
        if end == "tile_last_bit":
            assert (lf - tile0) % SC.TILE_BITS == SC.TILE_BITS - 1 and not c.pad
            assert (lf + B - 1 - tile0) // SC.TILE_BITS == ntiles        # ... and it ends in the overlap piece
        elif end == "next_tile_first_bit":
            assert (lf - tile0) % SC.TILE_BITS == 0 and (lf - tile0) // SC.TILE_BITS == ntiles - 1 and not c.pad
        elif end == "piece_end":
            assert nbits % 128 == 0 and (nbits - tile0) % SC.TILE_BITS != 0 and c.pad
        else:
            assert nbits % 128 == 0 and (nbits - tile0) == ntiles * SC.TILE_BITS and c.pad
            assert g0 + ntiles * SC.TILE_PIECES == pieces      # the last tile's overlap piece is the first past nu4
        if not c.pad:
            assert nbits % 32 != 0
    assert any(c.start >= 128 * 512 + 127 and (c.start >> 7) % 512 != 0 for _, c in SC.ALIGN_CASES)


def test_tiny_cases():
    assert {(c.n, c.fmt, c.T) for c in SC.TINY_CASES} == {(n, f, T) for n in (1, 2, 3) for f in SC.FORMATS for T in (1, 2)}
    for c in SC.TINY_CASES:
        assert c.n_phase == c.n and c.start % 128 == 127 and SC.word_bits(c) >= 3    # the first word spans two pieces


def test_structured_cases_fill_one_or_two_bins():
    assert sorted({SC.word_bits(c) for c in SC.STRUCTURED_CASES}) == [13, 16, 19, 22]
    assert {(SC.word_bits(c), c.fill) for c in SC.STRUCTURED_CASES} == {(B, f) for B in (13, 16, 19, 22) for f in ("ones", "alt")}
    assert {SC.instance_of(c.n, c.span, c.fmt)[0] for c in SC.STRUCTURED_CASES} == set(SC.MODES)
    for c in SC.STRUCTURED_CASES:
        words = SC.words_of(SC.case_bits(c), c.n, c.span, c.start, c.T)
        bins, counts = np.unique(words, return_counts=True)
        B = SC.word_bits(c)
        if c.fill == "ones":
            assert bins.tolist() == [2 ** B - 1] and counts.tolist() == [c.T]
        else:
            even = sum(1 << b for b in range(1, B, 2))        # a word that begins on an even bit: bits 1, 3, ... set
            assert sorted(bins.tolist()) == sorted([even, (2 ** B - 1) ^ even])
            assert sorted(counts.tolist()) == [c.T // 2, c.T - c.T // 2]


# ── window packing ──────────────────────────────────────────────────────────

def test_pack_instance_cases():
    assert [(c.n, c.fmt) for c in SC.PACK_INSTANCE_CASES] == [(n, f) for n in (1, 2, 3) for f in SC.FORMATS]
    assert (SC.PACK_Q0, SC.PACK_EXTRA_PITCH) == (3, 9)
    for c in SC.PACK_INSTANCE_CASES:
        spw = SC.steps_per_word(c.n)
        assert (c.nwin, c.n_phase) == (130, 1) and c.nwin == 2 * SC.PACK_SEQS + 2      # tiles of 64, 64 and 2 rows
        assert c.stride % 2 == 1 and np.gcd(c.stride, 128) == 1 and c.start % 2 == 1
        W = -(-c.N // spw)
        nchunks = -(-W // 4)
        assert nchunks == SC.PACK_CHUNKS + 1 and c.N % spw == 5 and W % 4 == 1         # a one-chunk tile, ragged word
        assert SC.pack_tile_bits(c.n) == (4096 if c.n < 3 else 3840)
        for ctile in (0, 1):
            off = SC.pack_offsets(c, ctile)
            assert sorted(set(off.tolist())) == list(range(128))
            assert set(off[:SC.PACK_SEQS].tolist()) | set(off[SC.PACK_SEQS:2 * SC.PACK_SEQS].tolist()) == set(range(128))
        # offset 127 in a full tile: the word of chunk 31, element 3 reads the row's last dword pair
        b = 127 + spw * c.n * (4 * 31 + 3)
        assert (b >> 5) + 1 < SC.PACK_ROW_DWORDS
        if c.n < 3:
            assert ((b >> 5), (b >> 5) + 1) == (130, 131) and SC.PACK_ROW_DWORDS == 132
    assert len({c.stride for c in SC.PACK_INSTANCE_CASES}) == 9


def test_pack_phase_and_piece_end_cases():
    assert {(c.n, c.fmt) for c in SC.PACK_PHASE_CASES} == {(n, f) for n in (2, 3) for f in ("bytes", "lsb")}
    for c in SC.PACK_PHASE_CASES:
        assert c.n_phase == c.n and c.nwin * c.n_phase > 2 * SC.PACK_SEQS and not c.pad
        assert SC.pack_nbits(c) % 32 != 0
    assert {(c.n, c.fmt) for c in SC.PACK_PIECE_END_CASES} == {(n, f) for n in (2, 3) for f in ("bytes", "lsb")}
    for c in SC.PACK_PIECE_END_CASES:
        assert c.pad and SC.pack_nbits(c) % 128 == 0 and c.start >= 0
        # the last window ends on the capture's last bit: its funnel's second piece lies past the capture
        assert c.start + (c.nwin - 1) * c.stride + c.N * c.n == SC.pack_nbits(c)

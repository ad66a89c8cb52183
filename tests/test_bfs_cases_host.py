"""tests/bfs_cases.py on the CPU: the product's host BFS (cvd_enumerate) equals the Python
restatement at the codes that test_gpu_bfs_edges.py gives the GPU search (so the GPU file's
reference is the contract, and a failure there lies in csrc/cvd_bfs.hip); the state counts and
level sizes the cases were chosen by; and every precondition the GPU file relies on, from the
reference alone.  The argument checks of cvd_enumerate_device that return before any device call
run here too."""
import ctypes

import numpy as np
import pytest

import bfs_cases as BC

CVD_E_INVALID, CVD_E_UNSUPPORTED = -1, -2

# the references' state counts and level sizes, recomputed (the counts of the issue's throw-away
# BFS for 41/47, 41/44, 41/42 and 101/111 are confirmed)
ANCHORS = {
    "m2": (31, [1, 2, 4, 4, 8, 4, 4, 4]),
    "m2b": (5, [1, 2, 2]),
    "m3": (435, [1, 2, 4, 8, 16, 28, 40, 60, 56, 88, 76, 32, 24]),
    "m4": (24_975, [1, 2, 4, 8, 16, 32, 64, 128, 248, 480, 824, 1352, 1936, 2296, 2464, 2592, 2752, 2496, 2032, 1560,
                    1256, 808, 480, 448, 288, 144, 64, 24, 32, 48, 32, 32, 16, 16]),
    "m4b": (12_815, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 832, 1280, 1776, 2520, 1872, 1848, 640, 384, 384, 128, 128]),
    "m5a": (9_727, [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 844, 1336, 1824, 1612, 1384, 736, 344, 176, 128, 192, 128]),
    "m5b": (14_573, [1, 2, 4, 8, 16, 32, 64, 128, 256, 450, 816, 1352, 1612, 1760, 1744, 1712, 1768, 992, 688, 400,
                     256, 224, 160, 96, 32]),
    "m5c": (29_327, [1, 2, 4, 8, 16, 32, 64, 128, 248, 488, 808, 1248, 1928, 2760, 3376, 3684, 3456, 3160, 2376, 1552,
                     1072, 908, 656, 432, 352, 248, 160, 64, 32, 32, 16, 16]),
    "m6a": (3_427, [1, 2, 4, 8, 16, 32, 64, 128, 256, 448, 784, 840, 620, 224]),
    "m6b": (29_791, [1, 2, 4, 8, 16, 32, 64, 80, 100, 124, 248, 496, 992, 784, 768, 736, 820, 1430, 2476, 3668, 6574,
                     10368]),
    "r23": (1_807, [1, 2, 4, 8, 16, 32, 64, 128, 176, 320, 240, 192, 208, 96, 96, 64, 32, 48, 16, 16, 16, 32]),
    "r23b": (14_691, [1, 2, 4, 8, 16, 32, 64, 128, 256, 440, 760, 1192, 1492, 1664, 1772, 1768, 1404, 880, 744, 560,
                      384, 272, 288, 208, 112, 96, 80, 48, 16]),
}


def test_code_table(pkg, golden):
    _, meta = golden
    for name, gold in (("m2", "m2_75"), ("m2b", "m2_65"), ("m3", "m3_demo"), ("r23", "r23_m4")):
        c = meta["codes"][gold]
        assert (*BC.shape(name), BC.taps(name)) == (c["m"], c["k"], c["n"], c["taps"]), name
    for name, cfg in (("m2", "m2"), ("r23", "r23_m4")):
        cc = pkg.CONFIG_CODES[cfg]
        assert (*BC.shape(name), BC.taps(name)) == (cc["m"], cc["k"], cc["n"], cc["gen1"]), name
    assert BC.taps("m4") == [[[1, 0, 0, 1, 1]], [[1, 1, 0, 1, 1]]]      # octal 23, 33: delay 0 first
    assert {BC.shape(name) for name in BC.CODES} == BC.INSTANCES
    assert {BC.key_words(name) for name in BC.CODES} == {1, 2, 4, 8}
    assert BC.shape("r23b") == BC.shape("r23") == (4, 2, 3) and BC.taps("r23b") != BC.taps("r23")
    assert sorted(BC.RESTATED + list(BC.HOST_ONLY)) == sorted(BC.CODES) == sorted(ANCHORS)
    assert set(BC.NEW_CODES) <= set(BC.CODES)
    for big, small in BC.HOST_ONLY.items():
        assert small in BC.RESTATED and BC.shape(small) == BC.shape(big)
        assert ANCHORS[small][0] < ANCHORS[big][0]


def test_level_sizes_of_a_hand_made_table():
    # 0 -> 1, 2; 1 -> 2, 3; 2 -> 0, 1; 3 -> 4, 0; 4 -> 4, 4: levels {0}, {1, 2}, {3}, {4}
    nx = np.array([[1, 2], [2, 3], [0, 1], [4, 0], [4, 4]], np.int64)
    assert BC.level_sizes_of(nx) == [1, 2, 1, 1]
    with pytest.raises(AssertionError):
        BC.level_sizes_of(np.array([[0, 0], [0, 1]], np.int64))      # state 1 has no earlier parent
    with pytest.raises(AssertionError):
        # state 2 (child of 1) would come before state 3 (child of 0): not a discovery order
        BC.level_sizes_of(np.array([[1, 3], [2, 2], [0, 0], [0, 0]], np.int64))


@pytest.mark.parametrize("name,gold", [("m2", "m2_75"), ("m2b", "m2_65"), ("m3", "m3_demo"), ("r23", "r23_m4")])
def test_tables_of_against_the_goldens(pkg, golden, name, gold):
    """the states array and the next table by received word, as the goldens index them"""
    z, _ = golden
    ref = BC.host_ref(pkg, name)
    np.testing.assert_array_equal(ref.states, z[f"{gold}/states"])
    tr = z[f"{gold}/transitions"]
    np.testing.assert_array_equal(ref.next[tr[:, 0], tr[:, 2]], tr[:, 1])
    assert len(tr) == ref.next.size


@pytest.mark.parametrize("name", BC.RESTATED)
def test_host_bfs_equals_restatement(pkg, name):
    """the same states in the same order, the same transitions, the same levels"""
    host, rest = BC.host_ref(pkg, name), BC.restated_ref(name)
    assert host.S == rest.S
    np.testing.assert_array_equal(host.states, rest.states)
    np.testing.assert_array_equal(host.next, rest.next)
    assert host.level_sizes == rest.level_sizes


@pytest.mark.parametrize("name", sorted(BC.CODES))
def test_anchors(pkg, name):
    ref = BC.host_ref(pkg, name)
    assert (ref.S, list(ref.level_sizes)) == ANCHORS[name]
    assert ref.S == sum(ref.level_sizes) == len(ref.states) and ref.S <= 30_000 < BC.GPU_CAP
    assert ref.states.shape == (ref.S, 1 << BC.shape(name)[0]) and not ref.states[0].any()
    assert ref.states.min(axis=1).max() == 0                       # Eq. 5: every vector has a zero
    assert len(np.unique(ref.states, axis=0)) == ref.S             # distinct states
    assert ref.states.max() <= 15                                  # the kernels pack a metric into a nibble


# ── preconditions of test_gpu_bfs_edges.py, from the reference alone ────────

@pytest.mark.parametrize("name", BC.CHUNK_CODES)
def test_chunk_codes_have_levels_of_many_chunks(pkg, name):
    ref = BC.host_ref(pkg, name)
    G = max(BC.candidates(ref, j) for j in range(len(ref.level_sizes)))
    assert G >= 8 * BC.MIN_CHUNK
    # and a level of several chunks that still finds new states (states met again from a later chunk)
    assert any(BC.candidates(ref, j) >= 8 * BC.MIN_CHUNK and ref.level_sizes[j + 1] > BC.MIN_CHUNK
               for j in range(len(ref.level_sizes) - 1))
    assert BC.key_words(name) in (4, 8) or BC.shape(name) == (4, 2, 3)


def test_chunk_edge_level(pkg):
    ref = BC.host_ref(pkg, BC.CHUNK_EDGE_CODE)
    G = BC.chunk_edge_G(ref)
    assert G - 1 >= BC.MIN_CHUNK                # none of G - 1, G, G + 1 is clamped to the minimum
    j = [BC.candidates(ref, i) for i in range(len(ref.level_sizes))].index(G)
    assert 0 < ref.level_sizes[j + 1] and G == 1800 and j == 9
    # later levels are larger, so chunks of G also end inside a level
    assert max(BC.candidates(ref, i) for i in range(len(ref.level_sizes))) > 2 * G


def test_collision_cases(pkg):
    """collisions are certain by counting (4 * 2^bits < S) and the largest group of states that
    share a narrowed hash, judged generously, stays far below the retry-pass limit"""
    assert sorted(BC.key_words(name) for name, _ in BC.COLLISIONS) == [1, 2, 2, 4, 8]
    assert [name for name, _ in BC.COLLISIONS if BC.shape(name) == (4, 2, 3)] == ["r23b"]
    for name, bits in BC.COLLISIONS:
        S = BC.host_ref(pkg, name).S
        assert 4 * 2 ** bits < S, name
        assert BC.GROUP_FACTOR * S / 2 ** bits < 1000 < BC.MAX_RETRY_PASSES, name


def test_give_up_case(pkg):
    """one hash value for every state: a candidate of a late level walks past more states than
    there are retry passes"""
    assert BC.host_ref(pkg, BC.GIVE_UP_CODE).S > 8200 > 2 * BC.MAX_RETRY_PASSES


def test_capacity_level(pkg):
    assert BC.shape(BC.CAP_CODE)[0] == 5
    ref = BC.host_ref(pkg, BC.CAP_CODE)
    L, C, j = ref.level_sizes, BC.cumulative(ref), BC.cap_level(ref)
    assert 2 <= j < len(L) - 2 and C[-1] == ref.S
    assert L[j] <= C[j - 1]                                        # the issue's choice of j
    # the level that passes the cap fits the staging area at each cap used (no overflow stop)
    assert L[j] <= BC.stage_entries(C[j] - 1) and L[j + 1] <= BC.stage_entries(C[j])
    assert L[-1] <= BC.stage_entries(ref.S - 1)
    assert (j, C[j - 1], C[j], C[j + 1]) == (10, 1023, 1867, 3203)


def test_no_code_of_the_table_overflows_its_staging_area(pkg):
    """The staging-overflow stop needs a level with more new states than max(1024, cap + 1), cap >=
    the states of all levels before it.  No code of the table has such a level, so
    test_gpu_bfs_edges.py has no staging-overflow test; a code added with one should get it."""
    for name in BC.CODES:
        assert BC.staging_overflows(BC.host_ref(pkg, name)) == [], name


def test_memory_case(pkg):
    """1 MiB beyond the fixed reserve cannot hold S states: a state costs at least its key and a
    16-byte slot at load <= 0.6"""
    ref = BC.host_ref(pkg, BC.MEM_CODE)
    assert BC.MEM_EXTRA / (4 * BC.key_words(BC.MEM_CODE) + 16 / 0.6) < ref.S
    assert BC.MEM_BELOW_RESERVE < BC.MEM_RESERVE < BC.MEM_RESERVE + BC.MEM_EXTRA


# ── argument checks that return before any device call ──────────────────────

def _call(pkg, m, k, n, device=0, cap=1000, S=None):
    code = pkg.Code([[[1] * (m + 1)] * k] * n, m, k, n)
    return pkg.lib().cvd_enumerate_device(code.c, device, cap, 0, S, None, None, None, 0, None, None)


@pytest.mark.parametrize("m,k,n", [(1, 1, 2), (7, 1, 2), (8, 1, 2), (4, 1, 3), (3, 2, 3), (5, 2, 3), (4, 2, 2),
                                   (4, 1, 1)])
def test_refused_shapes(pkg, m, k, n):
    """shapes inside kMaxM = 8, kMaxK = 4, kMaxN = 8 that pick() has no kernels for"""
    assert (m, k, n) not in BC.INSTANCES
    S = ctypes.c_int64(123)
    assert _call(pkg, m, k, n, S=ctypes.byref(S)) == CVD_E_UNSUPPORTED
    assert S.value == 0
    assert "unsupported code shape" in pkg.lib().cvd_last_error().decode()
    with pytest.raises(pkg.CvdError, match="unsupported code shape"):
        pkg.enumerate_states_device([[[1] * (m + 1)] * k] * n, m, k, n)


def test_invalid_arguments(pkg):
    S = ctypes.c_int64(123)
    assert _call(pkg, 3, 1, 2, cap=0, S=ctypes.byref(S)) == CVD_E_INVALID
    assert _call(pkg, 3, 1, 2, cap=-5, S=ctypes.byref(S)) == CVD_E_INVALID
    assert _call(pkg, 3, 1, 2, device=-1, S=ctypes.byref(S)) == CVD_E_INVALID
    assert _call(pkg, 3, 1, 2, S=None) == CVD_E_INVALID
    assert pkg.lib().cvd_enumerate_device(None, 0, 1000, 0, ctypes.byref(S), None, None, None, 0, None, None) \
        == CVD_E_INVALID
    assert "bad cvd_enumerate_device arguments" in pkg.lib().cvd_last_error().decode()
    # a shape outside kMaxM is invalid, not unsupported, and zeroes S_out
    code = pkg.Code([[[1] * 10], [[1] * 10]], 9, 1, 2)
    assert pkg.lib().cvd_enumerate_device(code.c, 0, 1000, 0, ctypes.byref(S), None, None, None, 0, None, None) \
        == CVD_E_INVALID
    assert S.value == 0

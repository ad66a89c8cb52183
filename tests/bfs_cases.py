"""Cases of the GPU state enumeration (csrc/cvd_bfs.hip, cvd_enumerate_device) and their
references.  TEST INFRASTRUCTURE ONLY.

* CODES: at least one code per kernel instance that pick() accepts -- <m,1,2> for m = 2..6 (key
  widths NW = 1, 1, 2, 4, 8 words) and <4,2,3> (NW = 2) -- each with a complete enumeration of at
  most about 30,000 states.
* The reference has two layers: oracle.restatement.enumerate_markov_states_allzero (pinned to the
  reference project's goldens in test_oracle_golden.py) and the product's host BFS
  (pkg.enumerate_markov_states_allzero, cvd_enumerate).  RESTATED names the codes whose host BFS
  test_bfs_cases_host.py compares with the restatement; the largest code of a shape is compared
  with the host BFS alone where the pure-Python restatement would take more than a few seconds.
* tables_of / level_sizes_of derive, from either layer's result, what the GPU search must return:
  the states array, the next table by received word, the level sizes.
* The choices the GPU file depends on (chunk count, narrowed hash widths, capacity levels, the
  staging rule) are functions of the reference alone; test_bfs_cases_host.py asserts them.

test_gpu_bfs_edges.py runs these cases through cvd_enumerate_device."""
import functools
from collections import namedtuple

import numpy as np

# name: (m, k, n, taps): taps of delays 0..m as octal digits, delay 0 first (as POLYS in
# test_gpu_decode_shapes.py); outputs separated by "/", the inputs of one output by ","
CODES = {
    "m2": (2, 1, 2, "7/5"),                    # golden m2_75, CONFIG_CODES["m2"]
    "m2b": (2, 1, 2, "6/5"),                   # golden m2_65: 5 states, levels of 1 and 2 states
    "m3": (3, 1, 2, "17/13"),                  # golden m3_demo
    "m4": (4, 1, 2, "23/33"),
    "m4b": (4, 1, 2, "30/37"),
    "m5a": (5, 1, 2, "41/44"),
    "m5b": (5, 1, 2, "41/42"),
    "m5c": (5, 1, 2, "41/47"),
    "m6a": (6, 1, 2, "101/120"),
    "m6b": (6, 1, 2, "101/111"),
    "r23": (4, 2, 3, "21,17/35,12/14,32"),     # golden r23_m4, CONFIG_CODES["r23_m4"]
    "r23b": (4, 2, 3, "23,15/30,27/2,33"),
}
NEW_CODES = ["m4", "m4b", "m5a", "m5b", "m5c", "m6a", "m6b", "r23b"]          # no golden holds them
RESTATED = ["m2", "m2b", "m3", "m4", "m4b", "m5a", "m5b", "m6a", "r23"]   # host BFS == restatement
HOST_ONLY = {"m5c": "m5a", "m6b": "m6a", "r23b": "r23"}   # the largest of a shape: the smaller code restated
INSTANCES = {(2, 1, 2), (3, 1, 2), (4, 1, 2), (5, 1, 2), (6, 1, 2), (4, 2, 3)}    # pick() in cvd_bfs.hip
HOST_CAP = 200_000
GPU_CAP = 40_000           # cap of the GPU searches: above every S of the table, a set of 131,072 slots

MIN_CHUNK = 1024           # cvd_bfs.hip: chunk = max(1024, CVD_BFS_CHUNK)
MAX_RETRY_PASSES = 4096    # cvd_bfs.hip: "if (pass > 4096)" gives up with CVD_E_STATE
MEM_RESERVE = 512 << 20    # cvd_bfs.hip: avail = budget - chunk_bytes - (512 << 20)

CHUNK_CODES = ["m5c", "m6b", "r23b"]           # with CVD_BFS_CHUNK = MIN_CHUNK: >= 8 chunks in a level
CHUNK_EDGE_CODE = "m5b"                        # chunk = G, G - 1, G + 1 of chunk_edge_G
# (code, CVD_BFS_HASH_BITS): one code per key width NW = 1, 2, 4, 8 and the second rate-2/3 code
COLLISIONS = [("m3", 4), ("m4b", 7), ("m5a", 6), ("m6a", 5), ("r23b", 8)]
GROUP_FACTOR = 4           # the largest hash group judged as GROUP_FACTOR * S / 2^bits
GIVE_UP_CODE = "m5a"       # CVD_BFS_HASH_BITS = 1: one hash for every state, S > 2 * MAX_RETRY_PASSES
CAP_CODE = "m5a"
MEM_CODE = "m5c"
MEM_EXTRA = 1 << 20        # mem_bytes = MEM_RESERVE + MEM_EXTRA: room for fewer states than MEM_CODE has
MEM_BELOW_RESERVE = 256 << 20

Ref = namedtuple("Ref", "S states next level_sizes")


def shape(name):
    m, k, n, _ = CODES[name]
    return m, k, n


def key_words(name):
    """NW of the code's kernel instance: 2^m nibbles in 32-bit words"""
    M = 1 << CODES[name][0]
    return M // 8 if M >= 8 else 1


def taps(name):
    """taps[j][i][d] multiplies x[d] of input i in output j; d = 0 is the input bit"""
    m, k, n, spec = CODES[name]
    gen = [[[int(c) for c in format(int(g, 8), "0%db" % (m + 1))] for g in row.split(",")] for row in spec.split("/")]
    assert len(gen) == n and all(len(row) == k and all(len(t) == m + 1 for t in row) for row in gen), name
    return gen


def tables_of(states, transitions, m, n):
    """(states [S, 2^m] uint8, next [S, 2^n] int64 indexed by received word (bit j = output j)) of
    an enumerate_markov_states_allzero result, built as test_gpu_bfs_equals_host_bfs_m4_2335 does"""
    S = len(states)
    st = np.array(states, np.uint8).reshape(S, 1 << m)
    nx = np.full((S, 1 << n), -1, np.int64)
    for i, d in transitions.items():
        for j, rl in d.items():
            for r in rl:
                nx[i, sum(b << q for q, b in enumerate(r))] = j
    assert (nx >= 0).all() and (nx < S).all()
    return st, nx


def level_sizes_of(nx):
    """Level 0 is [state 0]; a state's level is one more than the level of the parent that first
    discovered it, the smallest i with the state in next[i].  Discovery order is level-monotone
    (asserted), so one pass over the states in order reads the levels off."""
    S, R = nx.shape
    first_parent = np.full(S, S, np.int64)
    np.minimum.at(first_parent, nx.reshape(-1), np.repeat(np.arange(S), R))
    level = np.zeros(S, np.int64)
    for j in range(1, S):
        assert first_parent[j] < j, "state %d is discovered by no earlier state" % j
        level[j] = level[first_parent[j]] + 1
    assert (np.diff(level) >= 0).all() and (np.diff(level) <= 1).all()
    return np.bincount(level).tolist()


def _ref(st, nx):
    st.setflags(write=False)
    nx.setflags(write=False)
    return Ref(len(st), st, nx, tuple(level_sizes_of(nx)))


@functools.lru_cache(maxsize=None)
def host_ref(pkg, name):
    """The product's host BFS (cvd_enumerate) of the code (computed once, read-only)."""
    m, k, n = shape(name)
    states, transitions, _ = pkg.enumerate_markov_states_allzero(taps(name), m, k, n, cap=HOST_CAP)
    return _ref(*tables_of(states, transitions, m, n))


@functools.lru_cache(maxsize=None)
def restated_ref(name):
    """oracle/restatement.py's BFS of the code (computed once, read-only)."""
    from oracle import restatement as R
    m, k, n = shape(name)
    states, transitions, _ = R.enumerate_markov_states_allzero(taps(name), m, k, n)
    return _ref(*tables_of(states, transitions, m, n))


def cumulative(ref):
    """C_j = states of levels 0..j"""
    return np.cumsum(ref.level_sizes).tolist()


# ── what the GPU file chooses from the reference ────────────────────────────

def candidates(ref, j):
    """G of level j: every (parent, received word) of the level is a candidate"""
    return ref.level_sizes[j] * ref.next.shape[1]


def chunk_edge_G(ref):
    """G of the first level with more than MIN_CHUNK candidates (so that G - 1 is no clamped chunk)"""
    return next(candidates(ref, j) for j in range(len(ref.level_sizes)) if candidates(ref, j) > MIN_CHUNK)


def stage_entries(cap):
    """Staging capacity of a search capped at `cap` while memory is plentiful (cvd_bfs.hip: scap =
    min(cap + 1, ...), then "stage = std::max<int64_t>(1024, scap <= 2^26 ? scap : scap / 2)")"""
    assert cap + 1 <= 1 << 26
    return max(1024, cap + 1)


def cap_level(ref):
    """The middle level j of the capacity stops"""
    return len(ref.level_sizes) // 2


def staging_overflows(ref):
    """[(j, cap)]: a search capped at cap = C_j completes level j and then finds more new states in
    level j + 1 than its staging area holds"""
    C = cumulative(ref)
    return [(j, C[j]) for j in range(len(C) - 1) if ref.level_sizes[j + 1] > stage_entries(C[j])]


def assert_complete(out, ref):
    """`out` (enumerate_states_device(..., with_tables=True)) is the reference's enumeration"""
    assert out["complete"]
    assert out["S"] == ref.S == sum(out["level_sizes"])
    assert out["level_sizes"] == list(ref.level_sizes)
    np.testing.assert_array_equal(out["states"], ref.states)
    assert out["next"].shape == ref.next.shape
    assert (out["next"] >= 0).all() and (out["next"] < ref.S).all()
    np.testing.assert_array_equal(out["next"], ref.next)


def assert_incomplete(out, ref, cap=None):
    """`out` is a certified lower bound: whole reference levels and a last level no larger than
    the reference's; returns the number of levels"""
    lv = out["level_sizes"]
    assert not out["complete"] and "states" not in out
    assert out["S"] <= ref.S and sum(lv) == out["S"]
    if cap is not None:
        assert cap < out["S"]
    assert 2 <= len(lv) <= len(ref.level_sizes)
    assert lv[:-1] == list(ref.level_sizes[:len(lv) - 1])
    assert 1 <= lv[-1] <= ref.level_sizes[len(lv) - 1]
    return len(lv)

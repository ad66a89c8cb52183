"""The GPU state enumeration (csrc/cvd_bfs.hip, cvd_enumerate_device) at every kernel instance,
chunk edge and stop, against the host BFS (cvd_enumerate), which test_bfs_cases_host.py pins to
the Python restatement at these codes.  Every comparison is exact: the states in discovery order,
the whole successor table, the level sizes element by element.

Kernel instances and the codes that launch them (tests/bfs_cases.py):

  bfs_claim_kernel<2,1,2>  NW 1   m2, m2b
  bfs_claim_kernel<3,1,2>  NW 1   m3
  bfs_claim_kernel<4,1,2>  NW 2   m4, m4b
  bfs_claim_kernel<5,1,2>  NW 4   m5a, m5b, m5c
  bfs_claim_kernel<6,1,2>  NW 8   m6a, m6b
  bfs_claim_kernel<4,2,3>  NW 2   r23, r23b

bfs_resolve_kernel / bfs_place_kernel run at NW = 1, 2, 4, 8.  Chunks of the real minimum (1,024
candidates, 8 and more per level) and chunks that end on, one short of and one past a level; the
hash narrowed to a few bits at every key width (the claim / resolve retry passes) and to one bit
(the give-up after 4,096 passes); the capacity stop at cap = S, S - 1, C_j, C_j - 1 with its exact
count; the memory-budget stop; max_levels below the level count, null outputs, a non-default
stream.  The staging-overflow stop has no case (no code of the table has a level that large:
test_bfs_cases_host.py) and the CVD_BFS_SECONDS stop has none on purpose (a wall-clock test)."""
import ctypes

import numpy as np
import pytest
import torch

import bfs_cases as BC

pytestmark = pytest.mark.gpu

KNOBS = ("CVD_BFS_CHUNK", "CVD_BFS_HASH_BITS", "CVD_BFS_SECONDS", "CVD_BFS_VERBOSE")
CVD_OK, CVD_E_CAPACITY = 0, -3
SENTINEL = -7_777_777


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    """no knob left over"""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)


def _enumerate(pkg, name, cap=BC.GPU_CAP, **kw):
    """cap = GPU_CAP unless the test is about the cap: the search sizes its hash set by the cap
    (here 131,072 slots, up to a quarter of them taken, so probe paths cross other states), and at
    the wrapper's default cap it would first allocate and clear most of the device memory"""
    m, k, n = BC.shape(name)
    return pkg.enumerate_states_device(BC.taps(name), m, k, n, device=0, cap=cap, **kw)


def _complete(pkg, name):
    """the whole enumeration with its tables, equal to the reference"""
    ref = BC.host_ref(pkg, name)
    out = _enumerate(pkg, name, with_tables=True)
    BC.assert_complete(out, ref)
    return out


@pytest.mark.parametrize("name", sorted(BC.CODES))
def test_complete_enumeration_every_instance(pkg, name):
    _complete(pkg, name)


# ── chunk edges ─────────────────────────────────────────────────────────────

@pytest.mark.parametrize("name", BC.CHUNK_CODES)
def test_minimum_chunk(pkg, monkeypatch, name):
    """levels of 8 and more chunks: a new state met again from a later chunk keeps its smallest
    candidate code, a state staged by chunk c is matched by chunk c + 1 through the staged key"""
    monkeypatch.setenv("CVD_BFS_CHUNK", str(BC.MIN_CHUNK))
    _complete(pkg, name)


@pytest.mark.parametrize("delta", [0, -1, 1])
def test_chunk_ends_at_a_level_end(pkg, monkeypatch, delta):
    """a chunk that ends exactly on a level, one candidate short of it (a last chunk of one
    candidate) and one candidate past it"""
    G = BC.chunk_edge_G(BC.host_ref(pkg, BC.CHUNK_EDGE_CODE))
    monkeypatch.setenv("CVD_BFS_CHUNK", str(G + delta))
    _complete(pkg, BC.CHUNK_EDGE_CODE)


# ── forced hash collisions ──────────────────────────────────────────────────

@pytest.mark.parametrize("name,bits", BC.COLLISIONS, ids=[f"{c}-{b}bits" for c, b in BC.COLLISIONS])
def test_forced_collisions_every_key_width(pkg, monkeypatch, name, bits):
    """many states per hash value: each is kept apart by the key compare over all NW words, a
    retry resumes past the slot of the state it collided with"""
    monkeypatch.setenv("CVD_BFS_CHUNK", str(BC.MIN_CHUNK))
    monkeypatch.setenv("CVD_BFS_HASH_BITS", str(bits))
    _complete(pkg, name)


def test_gives_up_after_the_retry_pass_limit(pkg, monkeypatch):
    """one hash value for all of more than 8,200 states: the search fails with the state error
    and returns no count"""
    monkeypatch.setenv("CVD_BFS_HASH_BITS", "1")
    with pytest.raises(pkg.CvdError, match=r"error -5: .*hash-collision retries"):
        _enumerate(pkg, BC.GIVE_UP_CODE)


# ── stops ───────────────────────────────────────────────────────────────────

def test_capacity_stops_are_exact(pkg):
    """the stop is the sum of whole levels through the first level that passes cap"""
    name = BC.CAP_CODE
    ref = BC.host_ref(pkg, name)
    L, C, j = ref.level_sizes, BC.cumulative(ref), BC.cap_level(ref)
    BC.assert_complete(_enumerate(pkg, name, cap=ref.S, with_tables=True), ref)
    out = _enumerate(pkg, name, cap=ref.S - 1, with_tables=True)
    assert BC.assert_incomplete(out, ref, cap=ref.S - 1) == len(L) and out["S"] == ref.S
    out = _enumerate(pkg, name, cap=C[j])
    assert BC.assert_incomplete(out, ref, cap=C[j]) == j + 2 and out["S"] == C[j + 1]
    out = _enumerate(pkg, name, cap=C[j] - 1)
    assert BC.assert_incomplete(out, ref, cap=C[j] - 1) == j + 1 and out["S"] == C[j]
    out = _enumerate(pkg, name, cap=1)
    assert BC.assert_incomplete(out, ref, cap=1) == 2 and out["S"] == 1 + L[1]


def test_memory_budget_stop(pkg, monkeypatch):
    """a budget with room for fewer states than the code has: a certified lower bound made of
    whole reference levels; a budget below the fixed reserve: an error and no bound"""
    monkeypatch.setenv("CVD_BFS_CHUNK", str(BC.MIN_CHUNK))
    ref = BC.host_ref(pkg, BC.MEM_CODE)
    out = _enumerate(pkg, BC.MEM_CODE, mem_bytes=BC.MEM_RESERVE + BC.MEM_EXTRA, with_tables=True)
    print("\n  memory stop:", out["S"], "of", ref.S, "states,", len(out["level_sizes"]), "levels")
    BC.assert_incomplete(out, ref)
    assert out["S"] < ref.S
    with pytest.raises(pkg.CvdError, match=r"error -4: .*not enough device memory"):
        _enumerate(pkg, BC.MEM_CODE, mem_bytes=BC.MEM_BELOW_RESERVE)


# ── the C ABI directly ──────────────────────────────────────────────────────

def _raw(pkg, name, cap, level_buf, max_levels, want_n_levels=True, stream=None, tables=False):
    """cvd_enumerate_device through ctypes: (rc, S_out, n_levels_out, states, next)"""
    m, k, n = BC.shape(name)
    code = pkg.Code(BC.taps(name), m, k, n)
    S, nl = ctypes.c_int64(SENTINEL), ctypes.c_int32(SENTINEL)
    st = np.zeros((cap, 1 << m), np.uint8) if tables else None
    nx = np.zeros((cap, 1 << n), np.int32) if tables else None
    rc = pkg.lib().cvd_enumerate_device(
        code.c, 0, cap, 0, ctypes.byref(S), st.ctypes.data if tables else None, nx.ctypes.data if tables else None,
        level_buf.ctypes.data if level_buf is not None else None, max_levels,
        ctypes.byref(nl) if want_n_levels else None, stream)
    return rc, S.value, nl.value, st, nx


def _level_buf():
    return np.full(48, SENTINEL, np.int64)


def test_max_levels_below_the_level_count(pkg):
    """level_sizes is written up to max_levels entries and no further, on a complete search and
    on a capacity stop (the partial level's entry included); n_levels_out counts every level"""
    name = BC.CAP_CODE
    ref = BC.host_ref(pkg, name)
    L, C, j = list(ref.level_sizes), BC.cumulative(ref), BC.cap_level(ref)
    assert len(L) < 48
    for ml in (0, 1, 3, len(L) - 1, len(L), len(L) + 1):
        buf = _level_buf()
        rc, S, nl, _, _ = _raw(pkg, name, BC.GPU_CAP, buf, ml)
        assert (rc, S, nl) == (CVD_OK, ref.S, len(L)), ml
        w = min(ml, len(L))
        assert buf[:w].tolist() == L[:w] and (buf[w:] == SENTINEL).all(), ml
    stop = L[:j + 2]                     # cap = C_j: levels 0 .. j + 1 reached
    for ml in (0, 1, 3, j + 1, j + 2, j + 3):
        buf = _level_buf()
        rc, S, nl, _, _ = _raw(pkg, name, C[j], buf, ml)
        assert (rc, S, nl) == (CVD_E_CAPACITY, C[j + 1], j + 2), ml
        w = min(ml, j + 2)
        assert buf[:w].tolist() == stop[:w] and (buf[w:] == SENTINEL).all(), ml


def test_null_level_outputs(pkg):
    name = BC.CAP_CODE
    ref = BC.host_ref(pkg, name)
    C, j = BC.cumulative(ref), BC.cap_level(ref)
    for with_buf, ml, want_nl in ((False, 0, False), (False, 16, False), (False, 16, True), (True, 48, False)):
        buf = _level_buf() if with_buf else None
        rc, S, nl, _, _ = _raw(pkg, name, BC.GPU_CAP, buf, ml, want_n_levels=want_nl)
        assert (rc, S, nl) == (CVD_OK, ref.S, len(ref.level_sizes) if want_nl else SENTINEL)
        if with_buf:
            assert buf[:len(ref.level_sizes)].tolist() == list(ref.level_sizes)
            assert (buf[len(ref.level_sizes):] == SENTINEL).all()
        buf = _level_buf() if with_buf else None
        rc, S, nl, _, _ = _raw(pkg, name, C[j], buf, ml, want_n_levels=want_nl)
        assert (rc, S, nl) == (CVD_E_CAPACITY, C[j + 1], j + 2 if want_nl else SENTINEL)
        if with_buf:
            assert buf[:j + 2].tolist() == list(ref.level_sizes[:j + 2]) and (buf[j + 2:] == SENTINEL).all()


def test_non_default_stream_and_current_device(pkg):
    """the search ordered on a torch stream gives the same tables; the caller's current device is
    the same after the call (the call sets `device` while it runs)"""
    name = "m5b"
    ref = BC.host_ref(pkg, name)
    current = torch.cuda.device_count() - 1        # another device than 0 where there is one
    stream = torch.cuda.Stream(device=0)           # the search runs on device 0
    assert stream.cuda_stream != 0
    with torch.cuda.device(current):
        buf = _level_buf()
        rc, S, nl, st, nx = _raw(pkg, name, ref.S, buf, 48, stream=ctypes.c_void_p(stream.cuda_stream), tables=True)
        assert torch.cuda.current_device() == current
        stream.synchronize()
    assert (rc, S, nl) == (CVD_OK, ref.S, len(ref.level_sizes))
    BC.assert_complete({"complete": True, "S": S, "level_sizes": buf[:nl].tolist(), "states": st, "next": nx}, ref)

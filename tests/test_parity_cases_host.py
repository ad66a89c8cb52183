"""The conditions on tests/parity_cases.py that test_gpu_parity_template_shapes.py relies
on, checked where no GPU is needed: the templates reach every (n, T0, T1) kernel instance
and every n = 3 window edge, the vectorised count is the oracle's, the junk-filled buffer
unpacks to the words it was made from, and the random sequences' counts differ, so that a
threshold at one sequence's own fraction separates them."""
import numpy as np
import pytest
import torch

import parity_cases as PC
from oracle import parity as OP
from test_gpu_parity import unpack_words


def all_cases():
    for n in (1, 2, 3):
        for index, tpl in enumerate(PC.TEMPLATES[n]):
            for N in PC.N_VALUES(n, PC.first_of(tpl)):
                yield n, index, tpl, N


@pytest.mark.parametrize("n", [1, 2])
def test_every_instance_bucket_and_group_edge_is_reached(n):
    want = [(T0, T1) for T1 in (0, 32) for T0 in (4, 8, 16, 32)]
    reached = {}
    for tpl in PC.TEMPLATES[n]:
        c0, c1, cz, T0, T1 = PC.group_counts(n, tpl)
        assert (T0, T1) not in reached, "one template per instance"
        reached[(T0, T1)] = (c0, c1, cz)
        assert cz <= 2 and c0 <= 32 and c1 <= 32 and len(set(tpl)) == len(tpl)
        assert all(0 <= j < n and s >= 0 for (j, s) in tpl)
        offs = {PC.offset(n, t) for t in tpl}
        for count, edges in ((c0, PC.G0_EDGES), (c1, PC.G1_EDGES), (cz, PC.ZERO_EDGES[n])):
            assert count == 0 or set(edges) <= offs, (tpl, edges)
    assert sorted(reached) == sorted(want) == sorted(PC.INSTANCE_KEYS)
    assert len(PC.TEMPLATES[n]) == 8
    counts = list(reached.values())
    assert any(c0 == 0 and c1 > 0 for c0, c1, _ in counts)               # only the (prev, prev2) pair
    zero_only = [t for t in PC.TEMPLATES[n] if PC.group_counts(n, t)[:2] == (0, 0)]
    assert zero_only == [[(0, 0)] if n == 1 else [(0, 0), (1, 0)]] and PC.first_of(zero_only[0]) == 0
    # the full templates: T0 = 32 and T1 = 32 without a padding slot
    assert reached[(32, 0)] == (32, 0, n) and reached[(32, 32)] == (32, 32, n)
    assert sorted(len(t) for t in PC.TEMPLATES[n])[-2:] == ([33, 65] if n == 1 else [34, 66])
    # T0 = 8 and 16 both with and without padding slots
    assert reached[(8, 32)][0] == 8 and reached[(8, 0)][0] < 8
    assert reached[(16, 32)][0] == 16 and reached[(16, 0)][0] == 9
    # the launch-shape template: every group, and the T0 = 4 instance with terms in it
    c0, c1, cz, T0, T1 = PC.group_counts(n, PC.ALL_GROUPS[n])
    assert 0 < c0 <= 4 and c1 > 0 and cz == n and (T0, T1) == (4, 32)


def test_n3_templates_have_each_property():
    tpls = PC.TEMPLATES[3]
    firsts = [PC.first_of(t) for t in tpls]
    counts = [PC.group_counts(3, t) for t in tpls]
    assert all(0 <= j < 3 and 0 <= s <= 54 for t in tpls for (j, s) in t)
    assert all(max(c) <= 32 for c in counts)
    assert {s for t in tpls for (_, s) in t} >= set(PC.N3_DELAYS)
    assert any(min(c) == 0 for c in counts)                             # an output without a term
    assert any(max(c) == 32 for c in counts)                            # a full output
    assert any(0 < f <= 7 for f in firsts)                              # the control
    assert any(40 < f <= 54 for f in firsts) and 54 in firsts           # head = 2
    assert 0 in firsts                                                  # head = 0
    assert any(10 < f <= 40 for f in firsts)                            # past the previous word, head = 1
    assert min(PC.group_counts(3, PC.ALL_GROUPS[3])) > 0 and PC.first_of(PC.ALL_GROUPS[3]) == 54


@pytest.mark.parametrize("n", [1, 2, 3])
def test_window_lengths_cover_the_chunk_pipeline(n):
    spw, cs = PC.spw_of(n), 4 * PC.spw_of(n)
    assert cs == {1: 128, 2: 64, 3: 40}[n]
    for tpl in PC.TEMPLATES[n]:
        first = PC.first_of(tpl)
        Ns = PC.N_VALUES(n, first)
        assert Ns == sorted(set(Ns)) and Ns[0] == 0 and Ns[-1] < 700
        assert {0, 1, first, first + 1} <= set(Ns)
        chunks = {((N + spw - 1) // spw + 3) // 4 for N in Ns}
        assert set(range(0, 7)) <= chunks                                # 0..6 chunks
        assert any(N > 0 and N % cs == 0 for N in Ns)                    # ends on a chunk
        assert any(N % cs != 0 and N % spw == 0 for N in Ns)             # on a word
        assert any(N % spw != 0 for N in Ns)                             # inside a word
        head = (first + cs - 1) // cs
        if head > 0:
            assert any(head > N // cs for N in Ns)                       # head > tail


def test_sat_counts_is_the_oracle_count():
    for n, index, tpl, N in all_cases():
        rng = PC.case_rng(n, index, N)
        words = PC.random_words(rng, 9, N, n)
        got = PC.sat_counts(words, n, tpl)
        assert got.dtype == np.int64
        for q in range(len(words)):
            s, tot = OP.satisfied_count(OP.streams_from_words(words[q], n), tpl)
            assert (got[q], max(0, N - PC.first_of(tpl))) == (s, tot), (n, index, N, q)


def test_foreign_buffer_unpacks_to_words_and_fills_the_rest():
    for n in (1, 2, 3):
        spw = PC.spw_of(n)
        for N in PC.N_VALUES(n, 11):
            rng = np.random.default_rng([n, N])
            words = PC.random_words(rng, 70, N, n)
            buf = PC.foreign_buffer(rng, words, n)
            rows = max(1, ((N + spw - 1) // spw + 3) // 4)
            assert buf.dtype == np.int32 and buf.shape == (rows, 70, 4)
            np.testing.assert_array_equal(unpack_words(torch.from_numpy(buf), n, N), words.T)
            # the bits outside steps [0, N): random, so about half of them are set
            flat = buf.view(np.uint32).transpose(1, 0, 2).reshape(70, -1).astype(np.uint64)   # [nseq, W]
            bits = (flat[:, :, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)
            junk = bits.copy().reshape(70, -1, 32)
            t = np.arange(rows * 4 * spw)
            live = np.zeros((rows * 4, 32), bool)
            for j in range(n):
                live[t[:N] // spw, n * (t[:N] % spw) + j] = True
            dead = junk[:, ~live]
            assert dead.size > 0 or (n != 3 and N == rows * 4 * spw)
            if dead.size >= 70 * 8:
                assert 0.35 < dead.mean() < 0.65, (n, N, dead.mean())
            if n == 3 and N > 0:
                top = junk[:, :, 30:]
                assert 0.35 < top.mean() < 0.65


def test_random_sequences_give_distinct_counts():
    """With anchors to spare (N > first + 8) the sequences' counts take at least three
    values: a threshold at one sequence's own fraction has sequences on both sides of it."""
    seen = 0
    for n, index, tpl, N in all_cases():
        first = PC.first_of(tpl)
        if N <= first + 8:
            continue
        words = PC.random_words(PC.case_rng(n, index, N), PC.NSEQ, N, n)
        sat = PC.sat_counts(words, n, tpl)
        assert len(set(sat.tolist())) >= 3, (n, index, N)
        assert sat.max() <= N - first
        seen += 1
    assert seen > 150

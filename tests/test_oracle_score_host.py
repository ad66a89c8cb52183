"""Pin oracle.c_oracle.Model.score_words (oc_score_words: the oracle's per-sequence loop over
a caller's received words) from two sides, so that the GPU tests of foreign streams
(test_gpu_foreign_streams.py) stand on a checked reference: against run_trials on the
oracle's own streams, and against a numpy restatement of Eq. 4-5, the row lookup and the
T_ref count on one stream of every foreign kind.  Everything is bit-exact; CPU only."""
import math

import numpy as np
import pytest

import foreign_streams as F
from oracle import c_oracle as C
from oracle import restatement as R

SEED = F.SEED


@pytest.mark.parametrize("name,N,learn_len", [("m2", 200, None), ("m6", 400, 30_000)])
def test_score_words_equals_run_trials(pkg, name, N, learn_len):
    cc = pkg.CONFIG_CODES[name]
    m, p, T = cc["m"], 0.05, 8
    c1, c2 = C.Code(cc["gen1"], m, 1, 2), C.Code(cc["gen2"], m, 1, 2)
    om = C.Model(c1, p, learn_len, 200, 1.0, SEED)
    assert om.kind == (0 if name == "m2" else 1)
    counts, want = om.run_trials(c1, c2, N, p, SEED, 0, T, sums=True)
    tag = C.lib().oc_grid_tag(N, p)
    words = np.stack([C.stream(c1 if sid % 2 == 0 else c2, N, p, SEED, tag, sid) for sid in range(2 * T)])
    got, stats = om.score_words(words)
    assert np.array_equal(got, want.reshape(2 * T, 2))
    assert [int((got[0::2, 0] > got[0::2, 1]).sum()), int((got[1::2, 0] <= got[1::2, 1]).sum())] == counts.tolist()
    assert stats.shape == (2 * T, 4)
    assert (stats[:, 0] <= N).all() and (stats[:, 3] <= stats[:, 2]).all() and (stats[:, 1] <= stats[:, 0]).all()
    if name == "m2":
        assert (stats[:, 0] == N).all() and (stats[:, 1] == 0).all()   # a dense model: every D_t is a row
    # a second call and a reordered batch give the same numbers: no state between sequences
    perm = np.arange(2 * T)[::-1]
    again, st2 = om.score_words(words[perm])
    assert np.array_equal(again, got[perm]) and np.array_equal(st2, stats[perm])


def test_score_words_rejects_bad_words(pkg):
    cc = pkg.CONFIG_CODES["m2"]
    om = C.Model(C.Code(cc["gen1"], 2, 1, 2), 0.05, None, 200, 1.0, SEED)
    with pytest.raises(ValueError):
        om.score_words(np.array([[0, 1, 4]]))
    with pytest.raises(ValueError):
        om.score_words(np.array([[0, -1, 2]]))
    with pytest.raises(ValueError):
        om.score_words(np.array([0, 1, 2]))


def _step_all(D, bm, nxt_flat):
    """Eq. 4-5 for all four received words at once: D [64] -> successors [4, 64]."""
    cand = (D[None, :, None] + bm).reshape(4, -1)             # [q, (s, U)]
    Dn = np.full((4, D.size), np.iinfo(np.int64).max, np.int64)
    for q in range(4):
        np.minimum.at(Dn[q], nxt_flat, cand[q])
    return Dn - Dn.min(axis=1, keepdims=True)


def restated(om, taps, words):
    """(lp, lr, stats) of one sequence: rows and log P1 from Model.rows(), log(1/S) for a
    vector that is no row, c = the words whose successor equals the observed word's; the
    terms added in t order, as oc_score_words adds them."""
    lp_tab, keys = om.rows()
    index = {bytes(row): i for i, row in enumerate(keys)}
    unseen = math.log(1.0 / om.S)
    out, nxt = R.encoder_tables(taps, 6, 1, 2)
    pop = np.array([0, 1, 1, 2], np.int64)
    bm = pop[out[None, :, :] ^ np.arange(4)[:, None, None]]   # [q, s, U]
    D = np.zeros(64, np.int64)
    lp = lr = 0.0
    stats = [0, 0, 0, 0]
    prev = True
    for t, rv in enumerate(words):
        i = index.get(bytes(D.astype(np.uint8)))
        succ = _step_all(D, bm, nxt.reshape(-1))
        c = int((succ == succ[rv]).all(axis=1).sum())
        lp += lp_tab[i, rv] if i is not None else unseen
        lr += math.log(c / 4)
        row = i is not None
        stats[0] += row
        stats[1] += row and not prev
        stats[2] += c > 1
        stats[3] += c > 1 and t > 0
        prev = row
        D = succ[rv]
    return lp, lr, stats


@pytest.mark.parametrize("dec", [(0o133, 0o171), (0o133, 0o133)], ids=["133_171", "133_133"])
def test_score_words_equals_numpy_restatement(dec):
    """One stream of every kind at N = 200 (splice at 80 and 130, burst of 40 at 50).  The
    second decoder has g1 = g2: every word shares its successor with three others, c = 4."""
    N, p = 200, 0.05
    om = C.Model(F.code(dec), p, 30_000, 200, 1.0, SEED, enum_cap=0)
    assert om.kind == 1
    words = F.kind_minor_words(dec, p, N, 1, cuts=(80, 130), burst=(50, 40))
    assert words.shape == (len(F.KINDS), N)
    sums, stats = om.score_words(words)
    for q, kind in enumerate(F.KINDS):
        lp, lr, st = restated(om, F.gens(dec), words[q])
        assert (sums[q, 0], sums[q, 1]) == (lp, lr), kind
        assert stats[q].tolist() == st, kind
    if dec[0] == dec[1]:
        assert (stats[:, 2] == N).all()
    else:
        assert (stats[:, 2] == 1).all() and (stats[:, 3] == 0).all()
        # the streams differ in what they exercise: a noiseless own-code stream leaves the rows
        # only in the transient from D_0 = 0 (a few constraint lengths: 5 * 7 steps and a
        # margin), random words almost never meet one
        by = dict(zip(F.KINDS, stats[:, 0]))
        assert by["clean"] >= N - 40 and by["random"] < 0.1 * N


def test_foreign_inputs_meet_their_conditions():
    """The GPU file's seven references, built here without a GPU: the stats of its inputs meet
    the conditions it asserts before it runs anything (foreign_streams.check_inputs)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(4) as ex:       # (the C calls release the GIL)
        refs = list(ex.map(lambda a: F.reference(*a), F.MODELS))
    for mid, (dec, p), (om, words, want, stats) in zip(F.IDS, F.MODELS, refs):
        assert om.kind == 1 and words.shape == (F.NSEQ, F.N) and not np.isnan(want).any()
        F.check_inputs(mid, dec, p, stats)


def test_tref_fast_streams_count_above_one(pkg):
    """What tests/test_gpu_tref_fast.py's docstring says of its own streams (the m = 6 pair,
    N = 768, 256 trials, p = 0.01 / 0.05 / 0.2): c = 2 at step 0 of every sequence, and c > 1
    at one later step in all, at p = 0.2 on an H2 sequence."""
    from concurrent.futures import ThreadPoolExecutor
    cc = pkg.CONFIG_CODES["m6"]
    c1, c2 = C.Code(cc["gen1"], 6, 1, 2), C.Code(cc["gen2"], 6, 1, 2)
    N, T = 768, 256

    def stats_at(p):
        om = C.Model(c1, p, 300_000, 200, 1.0, SEED)
        tag = C.lib().oc_grid_tag(N, p)
        words = np.stack([C.stream(c1 if sid % 2 == 0 else c2, N, p, SEED, tag, sid) for sid in range(2 * T)])
        return om.score_words(words)[1]

    with ThreadPoolExecutor(3) as ex:
        st = dict(zip((0.01, 0.05, 0.2), ex.map(stats_at, (0.01, 0.05, 0.2))))
    for p, s in st.items():
        assert (s[:, 2] - s[:, 3] == 1).all(), p
    assert st[0.01][:, 3].sum() == 0 and st[0.05][:, 3].sum() == 0
    late = np.nonzero(st[0.2][:, 3])[0]
    assert late.tolist() == [241] and st[0.2][241, 3] == 1      # sequence id 241: trial 120's H2 stream


@pytest.mark.parametrize("dec", [d for d, _ in F.MODELS[3:]], ids=F.IDS[3:])
def test_native_model_of_other_decoders_equals_oracle(pkg, dec):
    """The product's host learning for the decoders that only the foreign-stream tests use:
    the oracle's rows, bit for bit."""
    cap = 0 if dec[0] == dec[1] else 500_000
    mod = pkg.Model(pkg.Code(F.gens(dec), 6, 1, 2), 0.05, 30_000, 200, 1.0, SEED, enum_cap=cap)
    om = C.Model(F.code(dec), 0.05, 30_000, 200, 1.0, SEED, enum_cap=cap)
    lp, keys = mod.rows()
    olp, okeys = om.rows()
    assert mod.info()["kind"] == om.kind == 1
    np.testing.assert_array_equal(keys, okeys)
    assert np.array_equal(lp, olp)
    assert mod.info()["logp1_unseen"] == math.log(1.0 / om.S)


def test_pack_layout_equals_per_word_packing():
    """pack_layout against the per-step definition of the stream buffer (include/cvd.h)."""
    rng = np.random.default_rng(1)
    nseq, N = 5, 773
    words = rng.integers(0, 4, (nseq, N))
    lay = F.pack_layout(words)
    W = lay.shape[0] * 4
    assert W == 52 and lay.shape == (13, nseq, 4) and lay.dtype == np.uint32
    flat = lay.transpose(1, 0, 2).reshape(nseq, W).astype(np.int64)
    t = np.arange(N)
    assert np.array_equal((flat[:, t // 16] >> (2 * (t % 16))) & 3, words)
    assert (flat[:, (N + 15) // 16:] == 0).all() and flat[0, N // 16] >> (2 * (N % 16)) == 0

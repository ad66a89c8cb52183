"""cvd_parity_detect at every compiled instance and every window edge against the oracle's
count (oracle.parity.satisfied_count, vectorised as parity_cases.sat_counts): the sixteen
(T0, T1) kernels of n = 1 and n = 2 and the n = 3 kernel's 64-bit windows, at window lengths
of zero to six 16-byte chunks, over buffers whose unused bits are random; the launch shapes;
the limits of include/cvd.h; the path Detector.scan takes to it at every symbol phase; and
its agreement with cvd_parity_sweep.  Satisfied counts are integers and P̂ is the same IEEE
double division on both sides, so every comparison is exact, the threshold at equality
included."""
import numpy as np
import pytest
import torch

import parity_cases as PC
from oracle import parity as OP
from test_gpu_capture import JUNK, capture_bits, oracle_capture, raw_capture  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu


def device_buffer(rng, words, n):
    return torch.from_numpy(PC.foreign_buffer(rng, words, n)).cuda()


def detect(pkg, buf, n, N, nseq, n_h1, tpl, gamma, want_sat=True, counts=None):
    """(sat [nseq] or None, counts (s1, s2)) of one cvd_parity_detect call."""
    sat = torch.full((nseq,), -7, dtype=torch.int32, device="cuda") if want_sat else None
    c = pkg.parity_detect(buf, n, N, nseq, n_h1, tpl, gamma, sat=sat, counts=counts)
    return (sat.cpu().numpy().astype(np.int64) if want_sat else None), tuple(c.cpu().tolist())


def decisions(ph, n_h1, gamma):
    """(H1 sequences with P̂ >= gamma, H2 sequences without): comp_parity.py:120-128."""
    return int(np.sum(ph[:n_h1] >= gamma)), int(np.sum(~(ph[n_h1:] >= gamma)))


# ───────────────────────── every instance, every edge ────────────────────────

INSTANCES = [(n, i) for n in (1, 2, 3) for i in range(len(PC.TEMPLATES[n]))]


def instance_id(case):
    n, i = case
    if n == 3:
        return "n3_first%d" % PC.first_of(PC.TEMPLATES[3][i])
    return "n%d_T0_%d_T1_%d" % ((n,) + PC.group_counts(n, PC.TEMPLATES[n][i])[3:])


@pytest.mark.parametrize("case", INSTANCES, ids=instance_id)
def test_counts_and_threshold_at_every_window_edge(pkg, case):
    n, index = case
    tpl = PC.TEMPLATES[n][index]
    first = PC.first_of(tpl)
    H1, H2 = 70, 200                                     # the sequence the threshold sits on, and its H2 copy
    for N in PC.N_VALUES(n, first):
        rng = PC.case_rng(n, index, N)
        words = PC.random_words(rng, PC.NSEQ, N, n)
        words[H2] = words[H1]
        buf = device_buffer(rng, words, n)
        want = PC.sat_counts(words, n, tpl)
        ph = PC.fractions(want, N, first)
        gamma = float(ph[H1])
        assert ph[H2] == gamma and (N > first or gamma == 0.0)
        sat, counts = detect(pkg, buf, n, N, PC.NSEQ, PC.N_H1, tpl, gamma)
        assert np.array_equal(sat, want), (n, tpl, N, np.nonzero(sat != want)[0][:8])
        assert counts == decisions(ph, PC.N_H1, gamma), (n, tpl, N)
        # at equality the H1 sequence succeeds and its H2 copy fails; one ulp up both flip
        pair = buf[:, [H1, H2], :].contiguous()
        up = float(np.nextafter(gamma, 2.0))
        assert detect(pkg, pair, n, N, 2, 1, tpl, gamma)[1] == (1, 0), (n, tpl, N)
        assert detect(pkg, pair, n, N, 2, 1, tpl, up)[1] == (0, 1), (n, tpl, N)
        assert detect(pkg, buf, n, N, PC.NSEQ, PC.N_H1, tpl, up, want_sat=False)[1] == \
            decisions(ph, PC.N_H1, up), (n, tpl, N)


# ─────────────────────────────── launch shapes ──────────────────────────────

@pytest.mark.parametrize("n", [1, 2, 3])
def test_launch_shapes_accumulate_counts(pkg, n):
    """One wave and less, a wave's edge, a block's edge; the H1 / H2 border at 0, inside a
    wave and at nseq; no sat array; counts added to what the tensor held."""
    tpl = PC.ALL_GROUPS[n]
    first = PC.first_of(tpl)
    N = 3 * 4 * PC.spw_of(n) + 5
    rng = np.random.default_rng([7, n])
    words = PC.random_words(rng, 257, N, n)
    want = PC.sat_counts(words, n, tpl)
    ph = PC.fractions(want, N, first)
    gamma = float(np.median(ph))
    assert 0 < np.sum(ph >= gamma) < len(ph)
    prior = (1000, 2_000_000_000_000)
    for nseq in (1, 63, 64, 65, 256, 257):
        buf = device_buffer(rng, words[:nseq], n)
        for n_h1 in sorted({0, 37, nseq} - ({37} if nseq < 37 else set())):
            counts = torch.tensor(prior, dtype=torch.int64, device="cuda")
            _, got = detect(pkg, buf, n, N, nseq, n_h1, tpl, gamma, want_sat=False, counts=counts)
            s1, s2 = decisions(ph[:nseq], n_h1, gamma)
            assert got == (prior[0] + s1, prior[1] + s2), (n, nseq, n_h1)
    counts = torch.tensor(prior, dtype=torch.int64, device="cuda")
    assert detect(pkg, buf, n, N, 0, 0, tpl, gamma, want_sat=False, counts=counts)[1] == prior


# ─────────────────── limits, as include/cvd.h states them ───────────────────

LIMIT_N, LIMIT_NSEQ = 150, 5

ACCEPTED = [
    (1, [(0, 64)]), (1, [(0, 0), (0, 64)]),
    (2, [(0, 32)]), (2, [(1, 32)]), (2, [(1, 0), (0, 32), (1, 32)]),
    (3, [(0, 54)]), (3, [(1, 54)]), (3, [(2, 54)]), (3, [(0, 54), (1, 54), (2, 54), (1, 0)]),
    (3, [(1, s) for s in range(23, 55)]),                                # 32 terms on one output
    (2, [(0, 3), (0, 3), (1, 1)]),                                       # the pair cancels, first stays 3
]
REFUSED = [
    (1, [(0, 65)]), (2, [(0, 33)]), (2, [(1, 33)]), (3, [(0, 55)]),
    (1, [(0, -1)]), (2, [(1, -1)]), (3, [(2, -1)]),
    (1, [(1, 0)]), (2, [(2, 0)]), (3, [(3, 0)]), (2, [(-1, 1)]),
    (0, [(0, 0)]), (4, [(0, 0)]),
    (3, [(2, s) for s in range(33)]),                                    # 33 terms on one output
    (3, [(0, 1), (2, 55), (1, 1)]), (2, [(0, 1), (1, 1), (0, 40)]),      # one bad term among good ones
]
# repeated terms: CvdError or the oracle's count (where the repeats cancel), nothing else
REPEATS = [
    (1, [(0, 0), (0, 0)]), (1, [(0, 0), (0, 0), (0, 0)]), (2, [(0, 0), (1, 0), (1, 0)]),
    (2, [(1, 0), (1, 0), (0, 2)]), (2, [(1, 32), (1, 32), (0, 1)]), (1, [(0, 64), (0, 64), (0, 33), (0, 2)]),
    (1, [(0, 5)] * 32 + [(0, 2)]), (1, [(0, 5)] * 33), (2, [(0, 20)] * 33 + [(1, 1)]),
    (3, [(1, 54), (1, 54), (0, 0)]), (3, [(2, 11)] * 32 + [(0, 3)]), (3, [(2, 11)] * 33 + [(0, 3)]),
    (2, [(0, 1), (1, 3)] * 48), (2, [(0, 1), (1, 3)] * 48 + [(0, 0)]),
]


@pytest.fixture(scope="module")
def limit_buffers():
    out = {}
    for n in (1, 2, 3):
        rng = np.random.default_rng([3, n])
        words = PC.random_words(rng, LIMIT_NSEQ, LIMIT_N, n)
        out[n] = (words, device_buffer(rng, words, n))
    return out


@pytest.mark.parametrize("n,tpl", ACCEPTED, ids=lambda v: str(v)[:40])
def test_limits_accepted(pkg, limit_buffers, n, tpl):
    words, buf = limit_buffers[n]
    sat, _ = detect(pkg, buf, n, LIMIT_N, LIMIT_NSEQ, LIMIT_NSEQ, tpl, 0.5)
    assert np.array_equal(sat, PC.sat_counts(words, n, tpl))
    assert list(sat) == [OP.satisfied_count(OP.streams_from_words(w, n), tpl)[0] for w in words]


@pytest.mark.parametrize("n,tpl", REFUSED, ids=lambda v: str(v)[:40])
def test_limits_refused(pkg, limit_buffers, n, tpl):
    _, buf = limit_buffers[min(max(n, 1), 3)]
    counts = torch.tensor([5, 6], dtype=torch.int64, device="cuda")
    with pytest.raises(pkg.CvdError):
        pkg.parity_detect(buf, n, LIMIT_N, LIMIT_NSEQ, LIMIT_NSEQ, tpl, 0.5, counts=counts)
    with pytest.raises(pkg.CvdError):                                    # refused without sequences too
        pkg.parity_detect(buf, n, LIMIT_N, 0, 0, tpl, 0.5, counts=counts)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [5, 6]


@pytest.mark.parametrize("n,tpl", REPEATS, ids=lambda v: str(v)[:40])
def test_repeated_terms_raise_or_count_like_the_oracle(pkg, limit_buffers, n, tpl):
    words, buf = limit_buffers[n]
    try:
        sat, _ = detect(pkg, buf, n, LIMIT_N, LIMIT_NSEQ, LIMIT_NSEQ, tpl, 0.5)
    except pkg.CvdError:
        return
    assert list(sat) == [OP.satisfied_count(OP.streams_from_words(w, n), tpl)[0] for w in words]


# ─────────────────────── the scan's path at every phase ──────────────────────

SCAN_TEMPLATES = {1: [(0, 0), (0, 31), (0, 33), (0, 64)],                # the (prev, prev2) pair
                  2: [(0, 0), (1, 0), (1, 16), (0, 17), (1, 32), (0, 32)],
                  3: [(0, 0), (1, 11), (2, 44), (0, 54)]}                # head = 2


def window_words(bits, first_bit, N, n):
    """Received words [len(first_bit), N] of the windows that begin at the given capture bits."""
    idx = np.asarray(first_bit, np.int64)[:, None] + np.arange(N * n, dtype=np.int64)[None, :]
    b = bits[idx].reshape(len(first_bit), N, n).astype(np.int64)
    return (b << np.arange(n)).sum(axis=2)


@pytest.mark.parametrize("fmt", ["bytes", "lsb", "msb"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_packed_windows_at_every_phase(pkg, n, fmt):
    """pack_capture(n_phase = n) -> parity_detect: sequence i n_phase + f holds capture bits
    start + i stride + f ..., overlapping windows from a start that is not byte-aligned."""
    N, start, nwin = 4 * 4 * PC.spw_of(n) + 7, 13, 23
    stride = N * n // 3 + 1
    nbits = start + (nwin - 1) * stride + (n - 1) + N * n
    rng = np.random.default_rng([11, n])
    bits = rng.integers(0, 2, nbits).astype(np.uint8)
    raw = raw_capture(bits, fmt, rng)
    assert np.array_equal(capture_bits(raw, fmt, nbits), bits)
    det = pkg.Detector(1, n, 2, [[[1, 1, 1]]] * n, device=0)
    buf, got_nwin = det.pack_capture(raw, N, start=start, stride=stride, n_phase=n, format=fmt, nbits=nbits)
    assert got_nwin == nwin
    tpl = SCAN_TEMPLATES[n]
    sat, _ = detect(pkg, buf, n, N, nwin * n, nwin * n, tpl, 0.6)
    q = np.arange(nwin * n)
    words = window_words(bits, start + (q // n) * stride + q % n, N, n)
    assert np.array_equal(sat, PC.sat_counts(words, n, tpl))
    for i in (0, n, nwin * n - 1):
        assert sat[i] == OP.satisfied_count(OP.streams_from_words(words[i], n), tpl)[0]


def test_scan_parity_columns_at_both_phases(pkg, oracle_capture):
    o = oracle_capture["m2"]
    N, tpl = o["N"], SCAN_TEMPLATES[2]
    first = PC.first_of(tpl)
    assert first > 16 and PC.group_counts(2, tpl)[4] == 32
    res = o["det"].scan(o["model"], o["bits"], N, start=JUNK, n_phase=2, batch=5, parity_template=tpl)
    nwin = 2 * o["trials"]
    assert res["parity_sat"].shape == res["parity_frac"].shape == (nwin, 2)
    for f in range(2):
        words = window_words(o["bits"], JUNK + f + np.arange(nwin) * 2 * N, N, 2)
        if f == 0:
            assert np.array_equal(words, np.stack(o["streams"]))
        want = [OP.satisfied_count(OP.streams_from_words(w, 2), tpl) for w in words]
        assert np.array_equal(res["parity_sat"][:, f], [w[0] for w in want]), f
        assert np.array_equal(res["parity_frac"][:, f], [w[0] / w[1] for w in want]), f
    assert np.array_equal(res["logp1"][:, 0], o["sums"][:, 0])


# ─────────────────────── agreement with the sweep kernel ─────────────────────

SWEEP_SPAN = {1: 6, 2: 6, 3: 4}


def sweep_templates(n, span):
    """Five templates whose largest delay is the span."""
    rng = np.random.default_rng([5, n])
    out = [[(0, span)], [(j, s) for j in range(n) for s in range(span + 1)]]
    while len(out) < 5:
        picked = rng.random((n, span + 1)) < 0.4
        tpl = [(j, s) for j in range(n) for s in range(span + 1) if picked[j, s]]
        if tpl and PC.first_of(tpl) == span and tpl not in out:
            out.append(tpl)
    return out


@pytest.mark.parametrize("n", [1, 2, 3])
def test_sweep_mask_count_equals_detect_count(pkg, n):
    """include/cvd.h: the template term (output j, delay s) of cvd_parity_detect is mask bit
    n (span - s) + j of cvd_parity_sweep.  Both counts equal the oracle's at every phase."""
    span, N, start = SWEEP_SPAN[n], 2003, 13
    T = N - span
    nbits = start + (n - 1) + N * n
    bits = np.random.default_rng([13, n]).integers(0, 2, nbits).astype(np.uint8)
    swept = pkg.parity_sweep(bits, n, span, start=start, T=T, n_phase=n).cpu().numpy()
    det = pkg.Detector(1, n, 2, [[[1, 1, 1]]] * n, device=0)
    words = window_words(bits, start + np.arange(n), N, n)
    packed = [det.pack_capture(bits, N, start=start + f, nwin=1)[0] for f in range(n)]
    for tpl in sweep_templates(n, span):
        mask = pkg.template_mask(tpl, n, span)
        for f in range(n):
            want = OP.satisfied_count(OP.streams_from_words(words[f], n), tpl)
            assert want[1] == T
            sat, _ = detect(pkg, packed[f], n, N, 1, 1, tpl, 0.6)
            assert (int(sat[0]), int(swept[f, mask])) == (want[0], want[0]), (n, tpl, f)

"""The product's host noise_word (csrc/cvd_common.h: the host learning chain's and the generic
generator kernel's bit-sliced noise) against the numpy spec, word by word
(tests/noise_host_check.cpp, compiled with g++): the crafted thresholds of tests/noise_cases.py
-- a chosen bit decided at every plane 1..32 in both low-bit fillings, equal through plane 32,
and u + 1 -- in sequences below and above 2^32, the threshold edges, and the 30-bit valid mask
of n = 3.  The whole-model tests reach planes past 24 only by chance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import noise_cases as NC
from oracle import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "noise_host_check.cpp")
VALID = {2: 0xFFFFFFFF, 3: (1 << 30) - 1}
EDGES = [0, 1, 2 ** 24 - 1, 2 ** 24, 2 ** 31, 2 ** 32 - 1, 2 ** 32]


def _cases():
    """(seed, tag, seq_id, w, thr, valid)"""
    out = []
    for n in (2, 3):
        for base in (NC.BASE, NC.BASE_HI):
            for (q, w, b) in NC.TARGETS[n]:
                sid = NC.seq_of(q, base)
                u = NC.uniform_of(NC.SEED, NC.TAG, sid, w, b)
                out += [(NC.SEED, NC.TAG, sid, w, thr, VALID[n]) for _, thr, _ in NC.all_cases(u)]
        for thr in EDGES:
            for sid, w in ((0, 0), (5, 3), (NC.BASE_HI, 2 ** 20 + 1)):
                out.append((NC.SEED, NC.TAG, sid, w, thr, VALID[n]))
                out.append((12345, philox.LEARN_TAG, sid, w, thr, VALID[n] >> 7))   # a partial last word
    return out


def _spec(cases):
    cache, want = {}, []
    for seed, tag, sid, w, thr, valid in cases:
        if (seed, tag, sid, w) not in cache:
            cache[seed, tag, sid, w] = [int(x) for x in philox.noise_word_uniforms(seed, tag, sid, [w], 2)[0]]
        want.append(sum(1 << b for b, u in enumerate(cache[seed, tag, sid, w]) if u < thr) & valid)
    return want


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_host_noise_word_equals_spec(tmp_path):
    exe = str(tmp_path / "noise_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe, SRC])
    cases = _cases()
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr
    got = [int(x, 16) for x in out.stdout.split()]
    want = _spec(cases)
    assert len(got) == len(want) == len(cases)
    bad = [(c, hex(g), hex(w)) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:5]
    # the cases do what they are for: each crafted threshold sets the target bit as predicted
    i = 0
    for n in (2, 3):
        for base in (NC.BASE, NC.BASE_HI):
            for (q, w, b) in NC.TARGETS[n]:
                u = NC.uniform_of(NC.SEED, NC.TAG, NC.seq_of(q, base), w, b)
                for label, thr, flips in NC.all_cases(u):
                    assert cases[i][4] == thr and (got[i] >> b) & 1 == flips, (n, base, q, w, b, label)
                    i += 1
        i += 6 * len(EDGES)
    assert i == len(cases)
    thr_of = np.array([c[4] for c in cases])
    g = np.array(got)
    assert (g[thr_of == 0] == 0).all() and (g[thr_of == 2 ** 32] == np.array([c[5] for c in cases])[thr_of == 2 ** 32]).all()

"""bench.py's plain run and its --dump-outputs files: a plain run carries none of the --full
legs, --steps sets the timed steps, and the dumped counts, stream words and per-sequence sums
are what the library computes for the same global trial ids (bit for bit)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

N, B, P, SEED, STEPS = 1000, 4096, 0.092, 12345, 2


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_dumps_the_timed_outputs(pkg, tmp_path):
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "0", "--config", "m2", "--N", str(N), "--batch", str(B), "--p", str(P),
                        "--fused", "0", "--dump-outputs", out], timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["steps"] == STEPS and len(j["diagnostic"]["step_ms"]) == STEPS and j["ms_per_step"] > 0
    assert j["unit"] == "trials/s" and j["higher_is_better"] is True and j["value"] > 0
    for moved in ("cpu_baseline", "pd_match_vs_cpu", "c0_demo", "reference_call", "early_decision"):
        assert moved not in j, moved
    assert j["box"] is None
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ["counts", "counts_last_step", "streams_sample", "sums_sample"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20

    # the same trial ids through the library: step s of a one-p sweep takes trials [s B, (s + 1) B)
    cc = pkg.CONFIG_CODES["m2"]
    det = pkg.Detector(cc["k"], cc["n"], cc["m"], cc["gen1"], device=0)
    model = det.model(P, None, 200, 1.0, SEED)
    whole = det.run_trials(model, cc["gen1"], cc["gen2"], N, P, SEED, 0, STEPS * B)["counts"].cpu().numpy()
    last = det.run_trials(model, cc["gen1"], cc["gen2"], N, P, SEED, (STEPS - 1) * B, STEPS * B, return_sums=True)
    assert np.array_equal(got["counts"], whole.reshape(1, 2).astype(np.float64))
    assert np.array_equal(got["counts_last_step"], last["counts"].cpu().numpy().reshape(1, 2).astype(np.float64))
    assert 0 < whole[0] < STEPS * B                     # an informative point: Pd neither 0 nor 1
    # sums of the last step's sequences: H1 of trial t at row t, H2 at row B + t
    b = _bench()
    S = last["sums"]
    rows = np.random.default_rng(SEED).integers(0, 2 * B, size=min(2 * B, b.DUMP_SAMPLE_ROWS))
    full = np.concatenate([S[:, 0:2], S[:, 2:4]], axis=0)
    assert np.array_equal(got["sums_sample"], full[rows])
    # the last step's received words, generated here into the bench's layout
    g1, g2 = pkg.Code(cc["gen1"], cc["m"], cc["k"], cc["n"]), pkg.Code(cc["gen2"], cc["m"], cc["k"], cc["n"])
    tb, tag = (STEPS - 1) * B, pkg.grid_tag(N, P)
    buf = det.stream_buffer(N, 2 * B)
    det.generate(g1, N, P, SEED, tag, 2 * tb, 2, B, out=buf, q0=0, pitch=2 * B)
    det.generate(g2, N, P, SEED, tag, 2 * tb + 1, 2, B, out=buf, q0=B, pitch=2 * B)
    words = -(-N // (32 // cc["n"]))
    want = b.sample_words(buf, words, 2 * B, SEED)
    assert want.shape == (min(b.DUMP_SAMPLE_WORDS, words * 2 * B),)
    assert np.array_equal(got["streams_sample"], want.astype(np.float64))
    assert got["streams_sample"].min() >= 0 and got["streams_sample"].max() < 2.0 ** 32

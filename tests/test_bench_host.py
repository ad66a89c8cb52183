"""bench.py's sweep weighting (CPU, no GPU): the headline weighs the six p of the sweep
equally whatever --steps is (Pd_plotter.py:199-233 runs num_iter trials
at every p)."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PER_P_MS = [1974.0, 2348.0, 2629.0, 2737.0, 2672.0, 2632.0]   # profiles/r04d/perp6.json (detector only)


def test_per_p_value_independent_of_step_count():
    b = _bench()
    B = 2_621_440
    ref = B / (sum(PER_P_MS) / 6 * 1e-3)
    for steps in (6, 8, 12, 20, 25):
        ms = [PER_P_MS[s % 6] for s in range(steps)]
        v, cov = b.sweep_value(ms, 6, B, 1)
        assert v == pytest.approx(ref, rel=1e-12) and cov == list(range(6)), steps
        # the unweighted wall rate over-weights the p that get an extra step
        wall = steps * B / (sum(ms) * 1e-3)
        assert (steps % 6 == 0) == (wall == pytest.approx(ref, rel=1e-12))


def test_per_p_value_scales_with_ranks_and_reports_coverage():
    b = _bench()
    v1, _ = b.sweep_value(PER_P_MS, 6, 1000, 1)
    v8, _ = b.sweep_value(PER_P_MS, 6, 1000, 8)
    assert v8 == pytest.approx(8 * v1)
    v, cov = b.sweep_value(PER_P_MS[:4], 6, 1000, 1)     # fewer steps than p: the covered p only
    assert cov == [0, 1, 2, 3] and v == pytest.approx(1000 / (sum(PER_P_MS[:4]) / 4 * 1e-3))


def test_sweep_all_value_is_trials_over_time():
    b = _bench()
    v, cov = b.sweep_value([4000.0, 4100.0], 6, 655_360, 2, sweep_all=True)
    assert v == pytest.approx(2 * 6 * 655_360 / (4050.0 * 1e-3)) and cov == list(range(6))
    with pytest.raises(ValueError):
        b.sweep_value([], 6, 1, 1)


def test_full_is_off_by_default_and_outputs_are_float64(monkeypatch, tmp_path):
    """A plain command line asks for none of the --full legs; --dump-outputs files are float64,
    and the stream sample reads seeded (word, sequence) positions of the [W/4, pitch, 4] layout,
    never the padding words."""
    import numpy as np
    import torch
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = b.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path)])
    a = b.parse()
    assert a.full is True and a.dump_outputs == str(tmp_path)
    b.dump_outputs(str(tmp_path / "d"), {"counts": np.array([[3, 1 << 40]], dtype=np.int64)})
    c = np.load(tmp_path / "d" / "counts.npy")
    assert c.dtype == np.float64 and c.tolist() == [[3.0, float(1 << 40)]]
    W, pitch, words = 8, 5, 6                       # words 6 and 7 of a sequence are padding
    w, q = np.meshgrid(np.arange(W), np.arange(pitch), indexing="ij")
    val = np.where(w < words, w * 1000 + q, -1)     # word w of sequence q; padding is -1
    buf = torch.from_numpy(val.reshape(W // 4, 4, pitch).transpose(0, 2, 1).copy()).to(torch.int32)
    s = b.sample_words(buf, words, pitch, seed=5, count=64)
    assert s.shape == (words * pitch,) and np.array_equal(s, b.sample_words(buf, words, pitch, seed=5, count=64))
    assert set(s.tolist()) <= {ww * 1000 + qq for ww in range(words) for qq in range(pitch)}
    buf[0, 0, 0] = -2                               # int32 words read back as unsigned
    assert b.sample_words(buf, 1, 1, seed=5, count=4).tolist() == [float(2 ** 32 - 2)]


def test_box_record_parsing(monkeypatch):
    """The box record (bench.py box_identity / ClockSampler): the visible cards follow the
    HIP visibility list, and the medians under load parse rocm-smi's clock / power strings."""
    b = _bench()
    d = {"card0": {}, "card1": {}, "card2": {}, "system": {}}
    monkeypatch.delenv("CUDA_VISIBLE_DEVICES", raising=False)
    monkeypatch.delenv("ROCR_VISIBLE_DEVICES", raising=False)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "2")
    assert b._visible_cards(d) == ["card2"]
    monkeypatch.delenv("HIP_VISIBLE_DEVICES")
    assert b._visible_cards(d) == ["card0", "card1", "card2"]
    s = b.ClockSampler(period=1.0)
    s.samples = [{"card0": {"sclk clock speed:": "(2383Mhz)", "Current Socket Graphics Package Power (W)": "1344.0",
                            "Temperature (Sensor junction) (C)": "58.0", "Card SKU": "N/A"}},
                 {"card0": {"sclk clock speed:": "(2100Mhz)", "Current Socket Graphics Package Power (W)": "1300.0",
                            "Temperature (Sensor junction) (C)": "57.0"}},
                 {"card0": {"sclk clock speed:": "(2390Mhz)", "Current Socket Graphics Package Power (W)": "1350.0",
                            "Temperature (Sensor junction) (C)": "59.0"}}]
    med = s.summary()["median_under_load"]["card0"]
    assert med["sclk clock speed:"] == 2383.0
    assert med["Current Socket Graphics Package Power (W)"] == 1344.0
    assert med["Temperature (Sensor junction) (C)"] == 58.0
    assert "Card SKU" not in med

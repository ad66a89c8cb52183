#!/usr/bin/env python3
"""Device-event timing of the blind parity-check sweep (cvd_parity_sweep) on
one GPU: a 2^30-bit LSB-packed capture (128 MiB), n = 2, both symbol phases, at span 6
(B = 14: the histogram in LDS) and span 8 (B = 18: eight parts of it in LDS); --spans 9,10
adds B = 20 and B = 22 (global atomics), and CVD_SWEEP_GLOBAL_B=16 in the environment
times global atomics at every B >= 16.  Per shape, after warm-up:

  (a) cvd_parity_sweep (histogram kernel + Walsh-Hadamard passes, the memset included);
  (b) the same [2, 2^B] array composed from torch ops on the device: byte shifts to the
      sliding words, torch.bincount, reshape add/sub stages (the only other way to these
      numbers on the GPU); checked equal to (a);
  (c) a device-to-device copy of the capture's bytes (the floor of anything that reads it).

Prints one JSON line per shape and the device's clocks.

  python profiles/parity_sweep_run.py [--log2-bits 30] [--reps 5] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def event_ms(fn, reps):
    """Median and minimum device time of fn() over `reps` runs, one event pair each."""
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2], times[0]


def torch_sweep(cap, n, span, T, n_phase, chunk=1 << 24):
    """sat [n_phase, 2^B] of an LSB-packed capture from torch ops (start = 0, n = 2): the
    word that begins at bit p is bits (p & 7) .. of the four bytes from byte p >> 3."""
    assert n == 2
    B = n * (span + 1)
    size, mask = 1 << B, (1 << B) - 1
    nbytes = cap.numel()
    hist = torch.zeros((n_phase, size), dtype=torch.int64, device=cap.device)
    for b0 in range(0, nbytes, chunk):
        b1 = min(nbytes, b0 + chunk)
        seg = torch.zeros(b1 - b0 + 3, dtype=torch.int64, device=cap.device)
        seg[:min(nbytes, b1 + 3) - b0] = cap[b0:min(nbytes, b1 + 3)]
        w32 = seg[:-3] | (seg[1:-2] << 8) | (seg[2:-1] << 16) | (seg[3:] << 24)
        pos = 8 * torch.arange(b0, b1, dtype=torch.int64, device=cap.device)
        for f in range(n_phase):
            last = f + n * (T - 1)                       # first bit of the phase's last word
            for s in range(f, 8, n):
                words = (w32 >> s) & mask
                if 8 * (b1 - 1) + s > last:               # the capture's tail: words past the last anchor
                    words = words[pos + s <= last]
                hist[f] += torch.bincount(words, minlength=size)
    v = hist
    h = 1
    while h < size:                                       # WHT: reshape add/sub stages
        p = v.view(n_phase, -1, 2, h)
        v = torch.stack([p[:, :, 0, :] + p[:, :, 1, :], p[:, :, 0, :] - p[:, :, 1, :]], dim=2).reshape(n_phase, size)
        h *= 2
    return (T + v) >> 1


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower() and "GPU[0]" in ln]
    except (OSError, subprocess.TimeoutExpired):
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bits", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spans", type=lambda s: [int(x) for x in s.split(",")], default=[6, 8])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible: nothing is measured")
    pkg = load_package()
    L = pkg.lib()
    dev = torch.device("cuda", 0)
    nbits = 1 << a.log2_bits
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)
    cap = torch.randint(0, 256, (nbits // 8,), dtype=torch.uint8, device=dev, generator=gen)
    other = torch.empty_like(cap)
    n, n_phase = 2, 2
    global_b = max(16, int(os.environ.get("CVD_SWEEP_GLOBAL_B", "22")))   # csrc/cvd_sweep.hip kGlobalMinB
    props = torch.cuda.get_device_properties(dev)
    head = {"device": props.name, "CUs": props.multi_processor_count, "clocks": clocks()}
    print(json.dumps(head))
    lines = [head]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for span in a.spans:
        B = n * (span + 1)
        T = (nbits - (n_phase - 1) - B) // n + 1
        work = torch.empty(L.cvd_parity_sweep_workspace_bytes(n, span, n_phase), dtype=torch.uint8, device=dev)
        sat = torch.zeros((n_phase, 1 << B), dtype=torch.int64, device=dev)

        def native():
            pkg._lib.check(L.cvd_parity_sweep(ctypes.c_void_p(cap.data_ptr()), nbits, pkg.CAPTURE_LSB, n, span, 0, T,
                                              n_phase, ctypes.c_void_p(sat.data_ptr()),
                                              ctypes.c_void_p(work.data_ptr()), stream))

        native()                                          # warm-up; also the checked result
        torch.cuda.synchronize()
        first = sat.clone()
        want = torch_sweep(cap, n, span, T, n_phase)      # warm-up of (b)
        assert torch.equal(first, want), "torch composition and cvd_parity_sweep differ"
        a_med, a_min = event_ms(native, a.reps)
        b_med, b_min = event_ms(lambda: torch_sweep(cap, n, span, T, n_phase), max(2, a.reps // 2))
        other.copy_(cap)
        c_med, c_min = event_ms(lambda: other.copy_(cap), 2 * a.reps)
        line = {"log2_bits": a.log2_bits, "n": n, "span": span, "B": B, "T": T, "n_phase": n_phase,
                "regime": "lds" if B <= 15 else "global" if B >= global_b else "lds-parts",
                "sweep_ms": round(a_med, 3), "sweep_min_ms": round(a_min, 3),
                "torch_ms": round(b_med, 3), "torch_min_ms": round(b_min, 3),
                "copy_ms": round(c_med, 4), "copy_min_ms": round(c_min, 4),
                "torch_over_sweep": round(b_med / a_med, 1), "sweep_over_copy": round(a_med / c_med, 1),
                "words_per_s": round(n_phase * T / (a_med * 1e-3), 0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

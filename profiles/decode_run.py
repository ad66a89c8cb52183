#!/usr/bin/env python3
"""Device-event timing of the capture decoder (cvd_viterbi_decode) on one GPU:
m = 6 (133,171) over a synthetic LSB-packed capture of 2^28 bits (2^27 steps of random data,
encoded and sent through a BSC of p = 0.05 with torch ops on the device).  Per (block, warm,
depth) setting, after warm-up:

  (a) cvd_viterbi_decode (all five kernels and the memset), with its three counters and the
      decoded bits' distance to the data that was sent;
  (b) a device-to-device copy of the capture's bytes (the floor of anything that reads it).

Prints one JSON line per setting and the device's clocks.  "0:-1:-1" is the library's defaults.

  python profiles/decode_run.py [--log2-bits 28] [--reps 5] [--settings 0:-1:-1,4096:256:128] [--out FILE]
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


def synthetic_capture(gen, m, T, p, dev, seed=12345):
    """(LSB-packed capture bytes of 2 T bits, the T data bits): the encoder from state 0."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.randint(0, 2, (T,), dtype=torch.uint8, device=dev, generator=g)
    n = len(gen)
    sym = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[d:, j] ^= u[:T - d]
    flips = torch.rand((T, n), device=dev, generator=g) < p
    sym ^= flips.to(torch.uint8)
    nflips = int(flips.sum())
    del flips
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
    cap = (sym.reshape(-1, 8) * w).sum(dim=1, dtype=torch.uint8)
    return cap.contiguous(), u, nflips


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower() and "GPU[0]" in ln]
    except (OSError, subprocess.TimeoutExpired):
        return []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-bits", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--settings", default="0:-1:-1",
                    type=lambda s: [tuple(int(x) for x in t.split(":")) for t in s.split(",")])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible: nothing is measured")
    pkg = load_package()
    L = pkg.lib()
    dev = torch.device("cuda", 0)
    cc = pkg.CONFIG_CODES["m6"]
    n, m, gen = cc["n"], cc["m"], cc["gen1"]
    code = pkg.Code(gen, m, 1, n)
    nbits = 1 << a.log2_bits
    T = nbits // n
    cap, sent, nflips = synthetic_capture(gen, m, T, a.p, dev)
    assert cap.numel() * 8 == nbits and cap.numel() % 16 == 0
    other = torch.empty_like(cap)
    props = torch.cuda.get_device_properties(dev)
    head = {"device": props.name, "CUs": props.multi_processor_count, "clocks": clocks(), "log2_bits": a.log2_bits,
            "T": T, "p": a.p, "channel_flips": nflips}
    print(json.dumps(head), flush=True)
    lines = [head]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    w8 = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
    sent_packed = (sent.reshape(-1, 8) * w8).sum(dim=1, dtype=torch.uint8)
    other.copy_(cap)
    c_med, c_min = event_ms(lambda: other.copy_(cap), 2 * a.reps)
    for block, warm, depth in a.settings:
        wbytes = int(L.cvd_viterbi_workspace_bytes(n, m, T, block))
        work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        bits = torch.zeros((T + 31) // 32 * 4, dtype=torch.uint8, device=dev)
        stats = torch.zeros(9, dtype=torch.int64, device=dev)

        def native():
            pkg._lib.check(L.cvd_viterbi_decode(code.c, ctypes.c_void_p(cap.data_ptr()), nbits, pkg.CAPTURE_LSB, 0, T,
                                                block, warm, depth, ctypes.c_void_p(bits.data_ptr()),
                                                ctypes.c_void_p(stats.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                                                stream))

        native()                                          # warm-up; also the reported result
        torch.cuda.synchronize()
        s = stats.cpu().tolist()
        wrong = int(torch.count_nonzero(bits[:T // 8] != sent_packed))   # bytes with a wrong data bit
        a_med, a_min = event_ms(native, a.reps)
        line = {"block": s[6], "warm": s[7], "depth": s[8], "blocks": s[1], "forward_reruns": s[2],
                "trace_fixups": s[3], "errors": s[0], "p_hat": s[0] / (n * T), "wrong_data_bytes": wrong,
                "workspace_MiB": round(wbytes / 2 ** 20, 1),
                "decode_ms": round(a_med, 3), "decode_min_ms": round(a_min, 3),
                "copy_ms": round(c_med, 4), "copy_min_ms": round(c_min, 4),
                "decode_over_copy": round(a_med / c_med, 1),
                "capture_bits_per_s": round(nbits / (a_med * 1e-3), 0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del work
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

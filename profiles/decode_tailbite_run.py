#!/usr/bin/env python3
"""Device-event timing of the tail-biting frame decoder (cvd_viterbi_decode_frames_tailbiting and
_soft) on one GPU: F tail-biting frames of T steps each (random data, encoded
circularly) one behind the other in a synthetic capture, sent through a BSC of p = 0.05 with
torch ops on the device.  Per workload code:F:T and flavour, after one warm-up, median of `reps`
event pairs:

  (a) one cvd_viterbi_decode_frames_tailbiting[_soft] call over all F frames, with its totals,
      the time per frame-lap (stats[8] laps were run) and the number of frames with at least
      one wrong information bit;
  (b) the baseline: cvd_viterbi_decode_frames[_soft](CVD_FRAME_ANY, CVD_FRAME_ANY) over the same
      capture -- one lap's forward work and a one-chain trace, the library's only batched way
      before; its bits are weakest at the two ends of a frame, which its count of wrong frames
      shows.

With --placement the LDS / workspace table of §7.16 instead: m = 6 (133,171) hard frames of each
T under both placements of the decision words (CVD_TAILBITE_LDS_BYTES forces either).

Prints one JSON line per measurement and the device's clocks.

  python profiles/decode_tailbite_run.py [--workloads lte:1048576:40,lte:1048576:128,wimax:65536:2048]
                                         [--placement 64,128,512,1024,2048] [--reps 5] [--out FILE]
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

CODES = {"lte": ("133", "171", "165"), "wimax": ("171", "133"), "m6": ("133", "171")}   # octal
M = 6


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


def tailbiting_capture(gen, F, T, p, dev, seed=12345):
    """(channel bits uint8 [F * T * n], one per byte; the data bits [F, T]; the flips)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.randint(0, 2, (F, T), dtype=torch.uint8, device=dev, generator=g)
    n = len(gen)
    sym = torch.zeros((F, T, n), dtype=torch.uint8, device=dev)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[:, :, j] ^= torch.roll(u, d, dims=1)       # u_{t-d}, t - d taken mod T
    flips = torch.rand((F, T, n), device=dev, generator=g) < p
    sym ^= flips.to(torch.uint8)
    return sym.reshape(-1), u, int(flips.sum())


def pack_lsb(bits):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=bits.device)
    return (bits.reshape(-1, 8) * w).sum(dim=1, dtype=torch.uint8).contiguous()


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower() and "GPU[0]" in ln]
    except (OSError, subprocess.TimeoutExpired):
        return []


def workload(s):
    code, F, T = s.split(":")
    return code, int(F), int(T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="lte:1048576:40,lte:1048576:128,wimax:65536:2048",
                    type=lambda s: [workload(t) for t in s.split(",") if t])
    ap.add_argument("--placement", default="", type=lambda s: [int(t) for t in s.split(",") if t])
    ap.add_argument("--placement-frames", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible: nothing is measured")
    pkg = load_package()
    L = pkg.lib()
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    lines = []

    def emit(line):
        line["clocks"] = clocks()
        print(json.dumps(line), flush=True)
        lines.append(line)

    emit({"device": props.name, "CUs": props.multi_processor_count, "p": a.p, "reps": a.reps})
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731

    def buffers(n, F, T, wbytes, cols):
        w = (T + 31) // 32
        return (torch.empty((F, 4 * w), dtype=torch.uint8, device=dev),
                torch.empty((F, cols), dtype=torch.int32, device=dev),
                torch.zeros(9, dtype=torch.int64, device=dev),
                torch.empty(wbytes, dtype=torch.uint8, device=dev) if wbytes else None)

    for name, F, T in a.workloads:
        gen = [[pkg.octal_to_taps(g, M)] for g in CODES[name]]
        n = len(gen)
        code = pkg.Code(gen, M, 1, n)
        chan, sent, nflips = tailbiting_capture(gen, F, T, a.p, dev)
        nbits = chan.numel()
        assert nbits == F * T * n and nbits % 128 == 0
        w = (T + 31) // 32
        sent_rows = pack_lsb(torch.nn.functional.pad(sent, (0, 32 * w - T))).reshape(F, 4 * w)
        for flavour in ("hard", "soft"):
            soft = flavour == "soft"
            cap = pkg.soft_from_bits(chan, 64) if soft else pack_lsb(chan)
            twork = int(L.cvd_viterbi_tailbiting_workspace_bytes(n, M, T, F, int(soft)))
            bits, frames, stats, work = buffers(n, F, T, twork, 8)
            tail = (0, n * T, None, F, T, 0, ptr(bits), ptr(frames), ptr(stats), ptr(work), stream)

            def tailbiting():
                if soft:
                    pkg._lib.check(L.cvd_viterbi_decode_frames_tailbiting_soft(code.c, ptr(cap), nbits, *tail))
                else:
                    pkg._lib.check(L.cvd_viterbi_decode_frames_tailbiting(code.c, ptr(cap), nbits, pkg.CAPTURE_LSB, *tail))

            tailbiting()                                  # warm-up; also the reported result
            torch.cuda.synchronize()
            s = stats.cpu().tolist()
            wrong = int((bits != sent_rows).any(dim=1).sum())
            t_med, t_min = event_ms(tailbiting, a.reps)
            del bits, frames, stats, work

            fwork = int(L.cvd_viterbi_frames_workspace_bytes(n, M, T, F, int(soft)))
            fbits, fframes, fstats, fwk = buffers(n, F, T, fwork, 6)
            ftail = (0, n * T, None, F, T, -1, -1, ptr(fbits), ptr(fframes), ptr(fstats), ptr(fwk), stream)

            def baseline():
                if soft:
                    pkg._lib.check(L.cvd_viterbi_decode_frames_soft(code.c, ptr(cap), nbits, *ftail))
                else:
                    pkg._lib.check(L.cvd_viterbi_decode_frames(code.c, ptr(cap), nbits, pkg.CAPTURE_LSB, *ftail))

            baseline()
            torch.cuda.synchronize()
            fwrong = int((fbits != sent_rows).any(dim=1).sum())
            f_med, f_min = event_ms(baseline, a.reps)
            del fbits, fframes, fstats, fwk
            emit({"code": name, "flavour": flavour, "F": F, "T": T, "channel_flips": nflips,
                  "decoded": s[1], "distance": s[0], "errors": s[3], "counted": s[4], "p_hat": s[3] / s[4],
                  "fallback": s[6], "open": s[7], "laps": s[8], "laps_per_frame": round(s[8] / F, 4),
                  "workspace_MiB": round(twork / 2 ** 20, 1), "baseline_workspace_MiB": round(fwork / 2 ** 20, 1),
                  "tailbiting_ms": round(t_med, 3), "tailbiting_min_ms": round(t_min, 3),
                  "ns_per_frame_lap": round(t_med * 1e6 / s[8], 2),
                  "baseline_ms": round(f_med, 3), "baseline_min_ms": round(f_min, 3),
                  "baseline_ns_per_frame": round(f_med * 1e6 / F, 2),
                  "tailbiting_over_baseline": round(t_med / f_med, 3),
                  "per_lap_over_baseline": round(t_med / s[8] / (f_med / F), 3),
                  "frames_with_wrong_data": wrong, "baseline_frames_with_wrong_data": fwrong})
            del cap
        del chan, sent, sent_rows

    # the placement of the decision words: dynamic LDS against the wave's slice of the workspace
    if a.placement:
        gen = [[pkg.octal_to_taps(g, M)] for g in CODES["m6"]]
        n, F = 2, a.placement_frames
        code = pkg.Code(gen, M, 1, n)
        for T in a.placement:
            chan, _, _ = tailbiting_capture(gen, F, T, a.p, dev)
            cap, nbits = pack_lsb(chan), chan.numel()
            line = {"placement": True, "F": F, "T": T, "decision_bytes_per_frame": (T + 63) // 64 * 64 * 8}
            rows = {}
            for where, limit in (("lds", "32768"), ("workspace", "1")):
                os.environ["CVD_TAILBITE_LDS_BYTES"] = limit
                wbytes = int(L.cvd_viterbi_tailbiting_workspace_bytes(n, M, T, F, 0))
                assert (wbytes == 0) == (where == "lds")
                bits, frames, stats, work = buffers(n, F, T, wbytes, 8)
                tail = (0, n * T, None, F, T, 0, ptr(bits), ptr(frames), ptr(stats), ptr(work), stream)

                def call():
                    pkg._lib.check(L.cvd_viterbi_decode_frames_tailbiting(code.c, ptr(cap), nbits, pkg.CAPTURE_LSB, *tail))

                call()
                torch.cuda.synchronize()
                rows[where] = bits.clone()
                med, mn = event_ms(call, a.reps)
                line[where + "_ms"], line[where + "_min_ms"] = round(med, 3), round(mn, 3)
                line[where + "_laps"] = stats.cpu().tolist()[8]
                del bits, frames, stats, work
            del os.environ["CVD_TAILBITE_LDS_BYTES"]
            assert torch.equal(rows["lds"], rows["workspace"])
            line["lds_over_workspace"] = round(line["lds_ms"] / line["workspace_ms"], 3)
            emit(line)
            del chan, cap, rows
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

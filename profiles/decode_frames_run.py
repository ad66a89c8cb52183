#!/usr/bin/env python3
"""Device-event timing of the frame decoder (cvd_viterbi_decode_frames and _soft, DESIGN.md
§7.15) on one GPU: m = 6 (133,171), F terminated frames of T steps each (random data, m zero
tail bits, from state 0) one behind the other in a synthetic capture, sent through a BSC of
p = 0.05 with torch ops on the device.  Per shape F:T and flavour, after one warm-up:

  (a) one cvd_viterbi_decode_frames[_soft] call over all F frames (memset, forward, trace and,
      soft, count), median of `reps` event pairs, with its totals and the number of frames whose
      decoded bits differ from the data that was sent;
  (b) the same frames the way the library offered before: a loop of decode_capture[_soft]
      calls, one per frame, over the first `loop_frames` frames, wall clock (every call
      synchronises), scaled to F frames;
  (c) the ceiling: cvd_viterbi_decode[_soft] over the capture as one stream of F T steps (wrong
      at every frame boundary; only its time is read).

Prints one JSON line per shape and flavour and the device's clocks.

  python profiles/decode_frames_run.py [--shapes 1048576:128,65536:2048] [--reps 5] [--loop-frames 1024] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

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


def framed_capture(gen, m, F, T, p, dev, seed=12345):
    """(channel bits uint8 [F * T * n], one per byte; the data bits [F, T]; the flips)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.randint(0, 2, (F, T), dtype=torch.uint8, device=dev, generator=g)
    u[:, T - m:] = 0
    n = len(gen)
    sym = torch.zeros((F, T, n), dtype=torch.uint8, device=dev)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[:, d:, j] ^= u[:, :T - d]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1048576:128,65536:2048",
                    type=lambda s: [tuple(int(x) for x in t.split(":")) for t in s.split(",")])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-frames", type=int, default=1024)
    ap.add_argument("--p", type=float, default=0.05)
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
    props = torch.cuda.get_device_properties(dev)
    head = {"device": props.name, "CUs": props.multi_processor_count, "clocks": clocks(), "p": a.p, "reps": a.reps,
            "loop_frames": a.loop_frames}
    print(json.dumps(head), flush=True)
    lines = [head]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for F, T in a.shapes:
        chan, sent, nflips = framed_capture(gen, m, F, T, a.p, dev)
        nbits = chan.numel()
        assert nbits == F * T * n and nbits % 128 == 0
        w = (T + 31) // 32
        sent_rows = pack_lsb(torch.nn.functional.pad(sent, (0, 32 * w - T))).reshape(F, 4 * w)
        for flavour in ("hard", "soft"):
            soft = flavour == "soft"
            cap = pkg.soft_from_bits(chan, 64) if soft else pack_lsb(chan)
            wbytes = int(L.cvd_viterbi_frames_workspace_bytes(n, m, T, F, int(soft)))
            work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
            bits = torch.empty((F, 4 * w), dtype=torch.uint8, device=dev)
            frames = torch.empty((F, 6), dtype=torch.int32, device=dev)
            stats = torch.zeros(6, dtype=torch.int64, device=dev)
            tail = (0, n * T, None, F, T, 0, 0, ptr(bits), ptr(frames), ptr(stats), ptr(work), stream)

            def batched():
                if soft:
                    pkg._lib.check(L.cvd_viterbi_decode_frames_soft(code.c, ptr(cap), nbits, *tail))
                else:
                    pkg._lib.check(L.cvd_viterbi_decode_frames(code.c, ptr(cap), nbits, pkg.CAPTURE_LSB, *tail))

            batched()                                     # warm-up; also the reported result
            torch.cuda.synchronize()
            s = stats.cpu().tolist()
            wrong = int((bits != sent_rows).any(dim=1).sum())
            b_med, b_min = event_ms(batched, a.reps)
            del work

            # (b) one call per frame, as before: the capture is on the device and used in place
            k = min(F, a.loop_frames)
            one = (lambda o: pkg.decode_capture_soft(n, m, gen, cap, start=o, T=T)) if soft else \
                (lambda o: pkg.decode_capture(n, m, gen, cap, start=o, T=T, format="lsb", nbits=nbits))
            one(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(k):
                one(f * n * T)
            torch.cuda.synchronize()
            loop_ms = (time.perf_counter() - t0) * 1e3

            # (c) the capture as one stream
            steps = F * T
            sentry = "cvd_viterbi_soft_workspace_bytes" if soft else "cvd_viterbi_workspace_bytes"
            swork = torch.empty(int(getattr(L, sentry)(n, m, steps, 0)), dtype=torch.uint8, device=dev)
            sbits = torch.empty((steps + 31) // 32 * 4, dtype=torch.uint8, device=dev)
            sstats = torch.zeros(11, dtype=torch.int64, device=dev)

            def streamed():
                if soft:
                    pkg._lib.check(L.cvd_viterbi_decode_soft(code.c, ptr(cap), nbits, 0, steps, 0, -1, -1, ptr(sbits),
                                                             ptr(sstats), ptr(swork), stream))
                else:
                    pkg._lib.check(L.cvd_viterbi_decode(code.c, ptr(cap), nbits, pkg.CAPTURE_LSB, 0, steps, 0, -1, -1,
                                                        ptr(sbits), ptr(sstats), ptr(swork), stream))

            streamed()
            torch.cuda.synchronize()
            s_med, s_min = event_ms(streamed, a.reps)
            del swork, sbits
            line = {"flavour": flavour, "F": F, "T": T, "steps": steps, "channel_flips": nflips,
                    "decoded": s[1], "skipped": s[2], "distance": s[0], "errors": s[3], "counted": s[4],
                    "p_hat": s[3] / s[4], "frames_with_wrong_data": wrong, "workspace_MiB": round(wbytes / 2 ** 20, 1),
                    "frames_ms": round(b_med, 3), "frames_min_ms": round(b_min, 3),
                    "loop_frames": k, "loop_ms_measured": round(loop_ms, 1), "loop_ms_per_call": round(loop_ms / k, 4),
                    "loop_ms_scaled_to_F": round(loop_ms / k * F, 0),
                    "stream_ms": round(s_med, 3), "stream_min_ms": round(s_min, 3),
                    "frames_over_stream": round(b_med / s_med, 2), "loop_over_frames": round(loop_ms / k * F / b_med, 0),
                    "steps_per_s": round(steps / (b_med * 1e-3), 0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del cap, bits, frames
        del chan, sent, sent_rows
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

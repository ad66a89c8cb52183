#!/usr/bin/env python3
"""Device-event timing of the encoder (cvd_encode_frames) on one GPU.  Random
information bits made on the device; per workload, after a warm-up, median and minimum of `reps`
event pairs of

  (enc)   one cvd_encode_frames call into a preallocated capture;
  (copy)  a device-to-device copy of the same number of output bytes: the bound of the BYTES and
          SOFT formats, whose time is the write;
  (torch) the same capture composed from torch ops on the device: unpack the rows, XOR the shifted
          streams, stack, select the kept outputs, scale or repack.  Its result is compared with
          the library's at the timed size (they must be equal).

Workloads: the (133,171) stream of 2^27 steps in each format; 2^20 terminated frames of 128 steps,
SOFT, plain and at dvb:3/4; 2^20 tail-biting frames of 40 steps of (133,171,165), SOFT.

Prints one JSON line per measurement with the device's clocks.

  python profiles/encode_run.py [--steps-log2 27] [--frames-log2 20] [--reps 20] [--select 3,4] [--out FILE]
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

M = 6
CODES = {"133,171": ("133", "171"), "133,171,165": ("133", "171", "165")}
MODES = {"open": 0, "terminated": 1, "tail-biting": 2}
FORMATS = {"lsb": 0, "msb": 1, "bytes": 2, "soft": 3}
AMPLITUDE = 24


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


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower() and "GPU[0]" in ln]
    except (OSError, subprocess.TimeoutExpired):
        return []


def torch_encode(gen, rows, T, mode, keep, fmt):
    """The capture of frames one behind the other from torch ops: rows uint8 [F, 4w] on the device."""
    n, F, dev = len(gen), rows.shape[0], rows.device
    u = ((rows[:, :, None] >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1).reshape(F, -1)[:, :T]
    if mode == "terminated":
        u = torch.cat([u[:, :T - M], torch.zeros((F, M), dtype=torch.uint8, device=dev)], dim=1)
    head = u[:, T - M:] if mode == "tail-biting" else torch.zeros((F, M), dtype=torch.uint8, device=dev)
    past = torch.cat([head, u], dim=1)                        # u_{t-d} at column M + t - d
    streams = []
    for j in range(n):
        s = None
        for d in range(M + 1):
            if gen[j][0][d]:
                x = past[:, M - d:M - d + T]
                s = x if s is None else s ^ x
        streams.append(s)
    c = torch.stack(streams, dim=2).reshape(F, n * T)
    if keep is not None:
        kept = torch.tensor([(keep[t % len(keep)] >> j) & 1 for t in range(T) for j in range(n)], dtype=torch.bool,
                            device=dev)
        c = c[:, kept]
    c = c.reshape(-1)
    if fmt == "bytes":
        return c
    if fmt == "soft":
        return ((2 * c.to(torch.int8) - 1) * AMPLITUDE).to(torch.int8)
    pad = (-c.numel()) % 8
    if pad:
        c = torch.cat([c, torch.zeros(pad, dtype=torch.uint8, device=dev)])
    order = torch.arange(8, device=dev, dtype=torch.uint8) if fmt == "lsb" else torch.arange(7, -1, -1, device=dev,
                                                                                            dtype=torch.uint8)
    return (c.reshape(-1, 8) << order).sum(dim=1, dtype=torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-log2", type=int, default=27)
    ap.add_argument("--frames-log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--select", default=None, type=lambda t: [int(x) for x in t.split(",")],
                    help="indices of the workloads to run, in the order above (default: all seven)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible: nothing is measured")
    pkg = load_package()
    L = pkg.lib()
    dec = __import__(pkg.__name__ + ".decode", fromlist=["puncture_pattern"])
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    lines = []

    def emit(line):
        line["clocks"] = clocks()
        print(json.dumps(line), flush=True)
        lines.append(line)

    emit({"device": props.name, "CUs": props.multi_processor_count, "reps": a.reps})
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Ts, Fs = 1 << a.steps_log2, 1 << a.frames_log2
    work = [("133,171", 1, Ts, "open", None, f) for f in ("lsb", "msb", "bytes", "soft")]
    work += [("133,171", Fs, 128, "terminated", None, "soft"), ("133,171", Fs, 128, "terminated", "dvb:3/4", "soft"),
             ("133,171,165", Fs, 40, "tail-biting", None, "soft")]
    if a.select is not None:
        work = [work[i] for i in a.select]
    g = torch.Generator(device=dev)
    g.manual_seed(12345)
    for name, F, T, mode, punct, fmt in work:
        gen = [[pkg.octal_to_taps(o, M)] for o in CODES[name]]
        n = len(gen)
        code = pkg.Code(gen, M, 1, n)
        keep = dec.puncture_pattern(punct, n) if punct else None
        span = n * T if keep is None else dec.punctured_bits(T, keep)
        w = (T + 31) // 32
        rows = torch.randint(0, 256, (F, 4 * w), dtype=torch.uint8, device=dev, generator=g)
        nout = F * span
        nbytes = nout if fmt in ("bytes", "soft") else (nout + 7) // 8
        rounded = (nbytes + 15) // 16 * 16
        out = torch.empty(rounded, dtype=torch.uint8, device=dev)
        src = torch.randint(0, 256, (rounded,), dtype=torch.uint8, device=dev, generator=g)
        dst = torch.empty_like(src)
        kb = bytes(keep) if keep else None

        def enc():
            rc = L.cvd_encode_frames(code.c, kb, len(keep) if keep else 0, ctypes.c_void_p(rows.data_ptr()), w, F, T,
                                     MODES[mode], 0, FORMATS[fmt], AMPLITUDE if fmt == "soft" else 0,
                                     ctypes.c_void_p(out.data_ptr()), nout, 0, span, None, None, stream)
            if rc != 0:
                raise SystemExit(L.cvd_last_error().decode())

        enc()
        want = torch_encode(gen, rows, T, mode, keep, fmt)
        torch.cuda.synchronize()
        equal = bool(torch.equal(out[:nbytes], want.view(torch.uint8)))
        del want
        dst.copy_(src)
        torch.cuda.synchronize()
        t_enc = event_ms(enc, a.reps)
        t_copy = event_ms(lambda: dst.copy_(src), a.reps)
        t_torch = event_ms(lambda: torch_encode(gen, rows, T, mode, keep, fmt), max(3, a.reps // 4))
        emit({"code": name, "F": F, "T": T, "mode": mode, "puncture": punct, "format": fmt, "out_bytes": nbytes,
              "info_bytes": F * 4 * w, "equal_to_torch": equal,
              "encode_ms": {"median": t_enc[0], "min": t_enc[1]}, "copy_ms": {"median": t_copy[0], "min": t_copy[1]},
              "torch_ms": {"median": t_torch[0], "min": t_torch[1]},
              "out_GBps": nbytes / t_enc[0] / 1e6, "steps_per_s": F * T / t_enc[0] * 1e3,
              "copy_over_encode": t_copy[0] / t_enc[0], "torch_over_encode": t_torch[0] / t_enc[0]})
        del rows, out, src, dst
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

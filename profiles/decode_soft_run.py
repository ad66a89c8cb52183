#!/usr/bin/env python3
"""Device-event timing, failure counters and information-bit errors of the soft-decision capture
decoder (cvd_viterbi_decode_soft) on one GPU: (171,133) over synthetic captures
of 2^27 steps of random data, encoded, sent as +-1 through Gaussian noise and quantised to int8
with torch ops on the device.  The noise level is given as p, the crossover probability of the
signs: sigma = 1 / Q^-1(p), so that the hard decoder beside it sees the BSC(p) of §7.11-7.12.

  time    cvd_viterbi_decode on the signs (LSB-packed; the yardstick) and cvd_viterbi_decode_soft
          on the values, both at their defaults: one warm-up, median and minimum of --reps runs
          between device events, time per step, the counters;
  ladder  per pattern (none, and the capture punctured and depunctured again with
          cvd_soft_depuncture), at L = 4096: forward reruns and traceback fix-ups at warm / depth
          = the hard decoders' defaults for that pattern times a ladder of factors (1 = the
          defaults as they are);
  ber     per pattern: the decoded bits' distance to the data that was sent, soft against the
          hard decoder on the signs of the same capture.

Prints one JSON line per run and the device's clocks.

  python profiles/decode_soft_run.py [--log2-steps 27] [--reps 5] [--p 0.02,0.05] [--scale 32]
      [--patterns none,dvb:3/4,dvb:7/8] [--time] [--ladder] [--factors 1,1.5,2,3,4] [--ber] [--out FILE]
"""
import argparse
import ctypes
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from __graft_entry__ import load_package  # noqa: E402
from decode_punctured_run import pack_lsb  # noqa: E402
from decode_run import clocks, event_ms  # noqa: E402


def transmit(gen, T, p, scale, dev, seed=12345):
    """(values [T, n] int8 after the channel, the T data bits): the encoder from state 0, +-1,
    noise of sigma = 1 / Q^-1(p), times `scale`, rounded and clipped to +-127."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.randint(0, 2, (T,), dtype=torch.uint8, device=dev, generator=g)
    n = len(gen)
    sym = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[d:, j] ^= u[:T - d]
    sigma = -1.0 / float(torch.special.ndtri(torch.tensor(p, dtype=torch.float64)))
    soft = torch.empty((T, n), dtype=torch.int8, device=dev)
    step = 1 << 24                                        # in pieces: the float noise of 2^28 values is 1 GiB
    for lo in range(0, T, step):
        y = 2.0 * sym[lo:lo + step].float() - 1.0
        y += sigma * torch.randn(y.shape, device=dev, generator=g)
        soft[lo:lo + step] = torch.clamp(torch.round(scale * y), -127, 127).to(torch.int8)
    return soft, u, sigma


def kept_mask(keep, T, n, dev):
    period = len(keep)
    col = torch.tensor([[(keep[c] >> j) & 1 for j in range(n)] for c in range(period)], dtype=torch.bool, device=dev)
    return col[torch.arange(T, device=dev) % period]


def padded(v, dev):
    """A flat tensor zero-padded to a multiple of 16 bytes."""
    pad = (-v.numel()) % 16
    return torch.cat([v, torch.zeros(pad, dtype=v.dtype, device=dev)]) if pad else v.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-steps", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", default=[0.02, 0.05], type=lambda s: [float(x) for x in s.split(",")])
    ap.add_argument("--scale", type=float, default=32.0, help="int8 units per unit of signal amplitude")
    ap.add_argument("--patterns", default=["none", "dvb:3/4", "dvb:7/8"], type=lambda s: s.split(","))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--ladder", action="store_true")
    ap.add_argument("--factors", default=[1, 1.5, 2, 3, 4], type=lambda s: [float(x) for x in s.split(",")])
    ap.add_argument("--ber", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU is visible: nothing is measured")
    pkg = load_package()
    dec = importlib.import_module(pkg.__name__ + ".decode")
    cli = importlib.import_module(pkg.__name__ + ".__main__")
    L = pkg.lib()
    dev = torch.device("cuda", 0)
    _, n, m, gen, _ = cli.code_of("oct:171,133")
    code = pkg.Code(gen, m, 1, n)
    T = 1 << a.log2_steps
    props = torch.cuda.get_device_properties(dev)
    head = {"device": props.name, "CUs": props.multi_processor_count, "clocks": clocks(), "T": T, "scale": a.scale}
    print(json.dumps(head), flush=True)
    lines = [head]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    work = torch.empty(int(L.cvd_viterbi_soft_workspace_bytes(n, m, T, 0)), dtype=torch.uint8, device=dev)
    bits = torch.zeros((T + 31) // 32 * 4, dtype=torch.uint8, device=dev)
    stats = torch.zeros(11, dtype=torch.int64, device=dev)
    pop = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int64, device=dev)
    out_ptr = [ctypes.c_void_p(t.data_ptr()) for t in (bits, stats, work)]

    def soft_call(cap, nvals, block, warm, depth):
        ptr = ctypes.c_void_p(cap.data_ptr())
        return lambda: pkg._lib.check(L.cvd_viterbi_decode_soft(code.c, ptr, nvals, 0, T, block, warm, depth, *out_ptr,
                                                                stream))

    def hard_call(keep, cap, nbits):
        ptr = ctypes.c_void_p(cap.data_ptr())
        if keep is None:
            return lambda: pkg._lib.check(L.cvd_viterbi_decode(code.c, ptr, nbits, pkg.CAPTURE_LSB, 0, T, 0, -1, -1,
                                                               *out_ptr, stream))
        kb = bytes(keep)
        return lambda: pkg._lib.check(L.cvd_viterbi_decode_punctured(code.c, kb, len(keep), ptr, nbits, pkg.CAPTURE_LSB,
                                                                     0, T, 0, -1, -1, *out_ptr, stream))

    def result(fn):
        fn()
        torch.cuda.synchronize()
        return stats.cpu().tolist()

    def wrong_bits(sent_packed):
        return int(pop[(bits[:T // 8] ^ sent_packed[:T // 8]).long()].sum())

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for p in a.p:
        soft, sent, sigma = transmit(gen, T, p, a.scale, dev)
        sent_packed = pack_lsb(sent, dev)
        for name in a.patterns:
            keep = None if name == "none" else pkg.puncture_pattern(name, n)
            if keep is None:
                cap, hard = padded(soft.reshape(-1), dev), pack_lsb((soft.reshape(-1) > 0).to(torch.uint8), dev)
                nbits, W0, D0 = n * T, dec.default_warm(m), dec.default_depth(m)
            else:
                kept = soft[kept_mask(keep, T, n, dev)]
                nbits, hard = kept.numel(), pack_lsb((kept > 0).to(torch.uint8), dev)
                cap = torch.empty((n * T + 15) // 16 * 16, dtype=torch.int8, device=dev)
                pkg._lib.check(L.cvd_soft_depuncture(ctypes.c_void_p(kept.data_ptr()), nbits, 0, bytes(keep), len(keep), n,
                                                     T, ctypes.c_void_p(cap.data_ptr()), stream))
                torch.cuda.synchronize()
                period, K = len(keep), dec.punctured_bits(len(keep), keep)
                W0, D0 = dec.default_warm_punctured(m, n, period, K), dec.default_depth_punctured(m, n, period, K)
                del kept
            base = {"pattern": name, "p": p, "sigma": round(sigma, 5), "capture_values": nbits,
                    "exact_zero_values": int((soft == 0).sum()) if keep is None else None}
            if a.time and keep is None:
                for which, fn in (("hard", hard_call(None, hard, nbits)), ("soft", soft_call(cap, n * T, 0, -1, -1))):
                    s = result(fn)                           # warm-up; also the reported result
                    med, mn = event_ms(fn, a.reps)
                    emit(dict(base, decoder=which, block=s[6], warm=s[7], depth=s[8], blocks=s[1], forward_reruns=s[2],
                              trace_fixups=s[3], metric=s[0], decode_ms=round(med, 3), decode_min_ms=round(mn, 3),
                              ns_per_step=round(med * 1e6 / T, 4)))
            if a.ladder:
                for f in a.factors:
                    s = result(soft_call(cap, n * T, 4096, math.ceil(f * W0), math.ceil(f * D0)))
                    emit(dict(base, factor=f, block=s[6], warm=s[7], depth=s[8], blocks=s[1], forward_reruns=s[2],
                              trace_fixups=s[3], metric=s[0], hard_errors=s[9], non_erased=s[10]))
            if a.ber:
                s = result(hard_call(keep, hard, nbits))
                emit(dict(base, decoder="hard", p_hat=s[0] / nbits, wrong_data_bits=wrong_bits(sent_packed),
                          forward_reruns=s[2], trace_fixups=s[3]))
                s = result(soft_call(cap, n * T, 4096, W0, D0))
                emit(dict(base, decoder="soft", p_hat=s[9] / s[10], wrong_data_bits=wrong_bits(sent_packed),
                          forward_reruns=s[2], trace_fixups=s[3], metric=s[0]))
            del cap, hard
        del soft
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

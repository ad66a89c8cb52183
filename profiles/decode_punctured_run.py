#!/usr/bin/env python3
"""Device-event timing and failure counters of the punctured capture decoder
(cvd_viterbi_decode_punctured) on one GPU: (171,133) over synthetic LSB-packed
captures of 2^27 steps of random data, encoded, sent through a BSC and punctured with torch ops
on the device.

  ladder  per pattern, at L = 4096: the forward reruns (a function of warm alone) and the
          traceback fix-ups (of depth alone) at warm / depth = the unpunctured defaults times
          1 + g e / K for a ladder of gains g (e = n period - K erased bits per period): the
          smallest g without a failure, times 1.5 and rounded up, is the header's gain;
  time    cvd_viterbi_decode on the unpunctured capture at its defaults (the yardstick) and the
          punctured call per pattern at the given gains (default: the library's), per p: one
          warm-up, median and minimum of --reps runs between device events, time per step, the
          counters, and the decoded bits' distance to the data that was sent.

Prints one JSON line per run and the device's clocks.

  python profiles/decode_punctured_run.py [--log2-steps 27] [--reps 5] [--patterns dvb:3/4,dvb:7/8]
      [--p 0.02,0.05] [--ladder] [--gains 1,1.5,2,3,4,6,8] [--warm-gain G --depth-gain G] [--out FILE]
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
from decode_run import clocks, event_ms  # noqa: E402


def encode(gen, T, p, dev, seed=12345):
    """(symbols [T, n] after the channel, the T data bits, channel flips [T, n]): the encoder from state 0."""
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
    return sym, u, flips


def pack_lsb(bits, dev):
    """LSB-packed bytes of a bit vector, zero-padded to 16 bytes."""
    pad = (-bits.numel()) % 128
    if pad:
        bits = torch.cat([bits, torch.zeros(pad, dtype=torch.uint8, device=dev)])
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
    return (bits.reshape(-1, 8) * w).sum(dim=1, dtype=torch.uint8).contiguous()


def punctured(sym, flips, keep, dev):
    """(capture bytes, capture bits, channel flips among the kept bits)."""
    T, n = sym.shape
    period = len(keep)
    col = torch.tensor([[(keep[c] >> j) & 1 for j in range(n)] for c in range(period)], dtype=torch.bool, device=dev)
    sel = col[torch.arange(T, device=dev) % period]
    kept = sym[sel]
    return pack_lsb(kept, dev), kept.numel(), int(flips[sel].sum())


def scaled(base, gain, e, K):
    return math.ceil(base * (K + gain * e) / K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-steps", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--p", default=[0.02, 0.05], type=lambda s: [float(x) for x in s.split(",")])
    ap.add_argument("--patterns", default=["dvb:3/4", "dvb:7/8"], type=lambda s: s.split(","))
    ap.add_argument("--ladder", action="store_true", help="the counters over a ladder of gains instead of the timing")
    ap.add_argument("--gains", default=[1, 1.5, 2, 3, 4, 6, 8], type=lambda s: [float(x) for x in s.split(",")])
    ap.add_argument("--warm-gain", type=float, default=None)
    ap.add_argument("--depth-gain", type=float, default=None)
    ap.add_argument("--skip-unpunctured", action="store_true", help="no yardstick run (for a kernel trace)")
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
    head = {"device": props.name, "CUs": props.multi_processor_count, "clocks": clocks(), "T": T}
    print(json.dumps(head), flush=True)
    lines = [head]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    wbytes = int(L.cvd_viterbi_workspace_bytes(n, m, T, 0))
    work = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    bits = torch.zeros((T + 31) // 32 * 4, dtype=torch.uint8, device=dev)
    stats = torch.zeros(10, dtype=torch.int64, device=dev)

    def run(keep, cap, nbits, block, warm, depth):
        ptr = [ctypes.c_void_p(t.data_ptr()) for t in (cap, bits, stats, work)]
        if keep is None:
            return lambda: pkg._lib.check(L.cvd_viterbi_decode(code.c, ptr[0], nbits, pkg.CAPTURE_LSB, 0, T, block, warm,
                                                               depth, ptr[1], ptr[2], ptr[3], stream))
        kb = bytes(keep)
        return lambda: pkg._lib.check(L.cvd_viterbi_decode_punctured(code.c, kb, len(keep), ptr[0], nbits,
                                                                     pkg.CAPTURE_LSB, 0, T, block, warm, depth, ptr[1],
                                                                     ptr[2], ptr[3], stream))

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for p in a.p:
        sym, sent, flips = encode(gen, T, p, dev)
        sent_packed = pack_lsb(sent, dev)
        todo = ([] if a.ladder or a.skip_unpunctured else [(None, None)]) + [(name, pkg.puncture_pattern(name, n)) for name in a.patterns]
        for name, keep in todo:
            if keep is None:
                cap, nbits, nflips = pack_lsb(sym.reshape(-1), dev), n * T, int(flips.sum())
                period, K, e = 1, n, 0
            else:
                cap, nbits, nflips = punctured(sym, flips, keep, dev)
                period, K = len(keep), dec.punctured_bits(len(keep), keep)
                e = n * period - K
            base = {"pattern": name or "none", "p": p, "capture_bits": nbits, "channel_flips": nflips}
            if a.ladder:
                for g in a.gains:
                    W, D = scaled(dec.default_warm(m), g, e, K), scaled(dec.default_depth(m), g, e, K)
                    fn = run(keep, cap, nbits, 4096, W, D)
                    fn()
                    torch.cuda.synchronize()
                    s = stats.cpu().tolist()
                    emit(dict(base, gain=g, block=s[6], warm=s[7], depth=s[8], blocks=s[1], forward_reruns=s[2],
                              trace_fixups=s[3], errors=s[0]))
                continue
            if keep is None or a.warm_gain is None:
                block, warm, depth = 0, -1, -1               # the library's defaults
            else:
                block = 4096
                warm = scaled(dec.default_warm(m), a.warm_gain, e, K)
                depth = scaled(dec.default_depth(m), a.depth_gain, e, K)
            fn = run(keep, cap, nbits, block, warm, depth)
            fn()                                             # warm-up; also the reported result
            torch.cuda.synchronize()
            s = stats.cpu().tolist()
            wrong = int(torch.count_nonzero(bits[:T // 8] != sent_packed[:T // 8]))   # bytes with a wrong data bit
            med, mn = event_ms(fn, a.reps)
            emit(dict(base, block=s[6], warm=s[7], depth=s[8], blocks=s[1], forward_reruns=s[2], trace_fixups=s[3],
                      errors=s[0], p_hat=s[0] / nbits, wrong_data_bytes=wrong, decode_ms=round(med, 3),
                      decode_min_ms=round(mn, 3), ns_per_step=round(med * 1e6 / T, 4),
                      warm_over_block=round(s[7] / s[6], 4)))
            del cap
        del sym, flips
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

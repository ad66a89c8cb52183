#!/usr/bin/env python3
"""Device-event timing of the punctured soft frame decoders (cvd_viterbi_decode_frames_soft_punctured,
_tailbiting_soft_punctured, _llr_punctured) on one GPU, each against
  (a) its unpunctured sibling on an already-depunctured capture of the same frames: the same steps
      and the same add-compare-select work, so the difference is the loader's, and
  (b) what a caller could do without them: a torch index_copy_ on the device that spreads the
      punctured values out into a capture of n T F bytes (zeros where nothing was sent, the buffer
      allocated and cleared outside the timed window), followed by the unpunctured call,
all in the same process, the three alternating: F terminated frames of T steps each of (171,133)
(random data, m zero tail bits, so s_0 = s_T = 0 and the frames are tail-biting as well) at
dvb:3/4, BPSK at amplitude A in Gaussian noise of sigma * A, rounded to int8, generated on the
device from a seed.  Per workload F:T, after one warm-up of each call, the median, the minimum and
the maximum of `reps` event pairs each.  The three results are compared before anything is timed.
Then what soft values buy: the wrong information bits of decode_frames_soft_punctured against
those of the punctured hard call (cvd_viterbi_decode_frames_punctured) on the signs of the same
values.

Prints one JSON line per measurement and the device's clocks.

  python profiles/decode_psoft01/decode_psoft_run.py [--workloads 1048576:128,65536:2048] [--sigma 0.61]
                                                     [--reps 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

M, OCT, PATTERN = 6, ("171", "133"), "dvb:3/4"


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "clk" in ln.lower() and "GPU[0]" in ln]
    except (OSError, subprocess.TimeoutExpired):
        return []


def terminated_values(gen, F, T, A, sigma, dev, seed=12345):
    """(int8 values [F, T * n]; the data bits uint8 [F, T], the last m zero)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    u = torch.randint(0, 2, (F, T), dtype=torch.uint8, device=dev, generator=g)
    u[:, T - M:] = 0
    n = len(gen)
    sym = torch.zeros((F, T, n), dtype=torch.uint8, device=dev)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[:, d:, j] ^= u[:, :T - d]                  # u_{t-d}; the encoder starts in state 0
    x = torch.randn((F, T, n), device=dev, generator=g) * (sigma * A)
    x += (2.0 * sym - 1.0) * A
    return x.round_().clamp_(-127, 127).to(torch.int8).reshape(F, T * n), u


def kept_columns(keep, n, T, dev):
    """The places n t + j of a frame's values that the pattern sends, ascending."""
    return torch.tensor([n * t + j for t in range(T) for j in range(n) if (keep[t % len(keep)] >> j) & 1],
                        dtype=torch.int64, device=dev)


def pack_lsb(bits):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=bits.device)
    return (bits.reshape(-1, 8) * w).sum(dim=1, dtype=torch.uint8).contiguous()


def wrong_bits(rows, sent_rows):
    x = (rows ^ sent_rows).reshape(-1)
    return int(sum(int(((x >> k) & 1).sum()) for k in range(8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="1048576:128,65536:2048",
                    type=lambda s: [tuple(int(x) for x in t.split(":")) for t in s.split(",") if t])
    ap.add_argument("--sigma", type=float, default=0.61)
    ap.add_argument("--amplitude", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
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
        print(json.dumps(line), flush=True)
        lines.append(line)

    emit({"device": props.name, "CUs": props.multi_processor_count, "clocks": clocks(), "sigma": a.sigma,
          "amplitude": a.amplitude, "pattern": PATTERN, "reps": a.reps})
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    gen = [[pkg.octal_to_taps(g, M)] for g in OCT]
    n = len(gen)
    code = pkg.Code(gen, M, 1, n)
    keep = pkg.puncture_pattern(PATTERN, n)
    kb, period = bytes(keep), len(keep)
    for F, T in a.workloads:
        full, sent = terminated_values(gen, F, T, a.amplitude, a.sigma, dev)
        cols = kept_columns(keep, n, T, dev)
        span, w = int(cols.numel()), (T + 31) // 32
        assert span == pkg.punctured_bits(T, keep)
        pcap = full[:, cols].contiguous().reshape(-1)             # the punctured capture: F frames of span values
        dep = torch.zeros_like(full).index_copy_(1, cols, pcap.view(F, span)).reshape(-1)   # (a)'s capture
        spread = torch.zeros((F, n * T), dtype=torch.int8, device=dev)                     # (b)'s buffer
        hard = (pcap > 0).to(torch.uint8)                         # the signs, one bit per byte
        del full
        pvals, dvals = pcap.numel(), dep.numel()
        assert pvals % 16 == 0 and dvals % 16 == 0
        sent_rows = pack_lsb(torch.nn.functional.pad(sent, (0, 32 * w - T))).reshape(F, 4 * w)
        fwork = int(L.cvd_viterbi_frames_workspace_bytes(n, M, T, F, 1))
        twork = int(L.cvd_viterbi_tailbiting_workspace_bytes(n, M, T, F, 1))
        lwork = int(L.cvd_viterbi_llr_workspace_bytes(n, M, T, F))
        work = torch.empty(max(fwork, twork, lwork, 16), dtype=torch.uint8, device=dev)
        llr = [torch.empty((F, 32 * w), dtype=torch.int16, device=dev) for _ in range(2)]
        bits = [torch.empty((F, 4 * w), dtype=torch.uint8, device=dev) for _ in range(2)]
        frames = [torch.empty((F, 8), dtype=torch.int32, device=dev) for _ in range(2)]
        stats = [torch.zeros(9, dtype=torch.int64, device=dev) for _ in range(2)]

        def out(i):
            return ptr(bits[i]), ptr(frames[i]), ptr(stats[i]), ptr(work), stream

        def spread_out():
            spread.index_copy_(1, cols, pcap.view(F, span))

        calls = {
            "frames": (
                lambda: L.cvd_viterbi_decode_frames_soft_punctured(code.c, kb, period, ptr(pcap), pvals, 0, span, None, F, T,
                                                                   0, 0, *out(0)),
                lambda c: L.cvd_viterbi_decode_frames_soft(code.c, ptr(c), dvals, 0, n * T, None, F, T, 0, 0, *out(1)), 6),
            "tailbiting": (
                lambda: L.cvd_viterbi_decode_frames_tailbiting_soft_punctured(code.c, kb, period, ptr(pcap), pvals, 0, span,
                                                                              None, F, T, 0, *out(0)),
                lambda c: L.cvd_viterbi_decode_frames_tailbiting_soft(code.c, ptr(c), dvals, 0, n * T, None, F, T, 0,
                                                                      *out(1)), 8),
            "llr": (
                lambda: L.cvd_viterbi_decode_frames_llr_punctured(code.c, kb, period, ptr(pcap), pvals, 0, span, None, F, T,
                                                                  0, 0, ptr(llr[0]), *out(0)),
                lambda c: L.cvd_viterbi_decode_frames_llr(code.c, ptr(c), dvals, 0, n * T, None, F, T, 0, 0, ptr(llr[1]),
                                                          *out(1)), 6),
        }
        for name, (new, old, nrec) in calls.items():
            def run_new():
                pkg._lib.check(new())

            def run_a():
                pkg._lib.check(old(dep))

            def run_b():
                spread_out()
                pkg._lib.check(old(spread))

            run_new()
            run_a()
            torch.cuda.synchronize()
            s_new = stats[0].cpu().tolist()
            assert torch.equal(bits[0], bits[1]) and s_new == stats[1].cpu().tolist()
            assert torch.equal(frames[0].reshape(-1)[:F * nrec], frames[1].reshape(-1)[:F * nrec])
            if name == "llr":
                assert torch.equal(llr[0], llr[1])
            new_wrong = wrong_bits(bits[0], sent_rows) if name == "frames" else None
            run_b()
            torch.cuda.synchronize()
            assert torch.equal(spread.reshape(-1), dep) and torch.equal(bits[0], bits[1])
            tn, ta, tb, tg = [], [], [], []
            for _ in range(a.reps):                              # alternating: all see the same neighbours
                tn.append(event_ms(run_new))
                ta.append(event_ms(run_a))
                tb.append(event_ms(run_b))
                tg.append(event_ms(spread_out))
            for t in (tn, ta, tb, tg):
                t.sort()
            med = lambda t: t[len(t) // 2]   # noqa: E731
            line = {"call": name, "code": ",".join(OCT), "F": F, "T": T, "span": span, "decoded": s_new[1],
                    "distance": s_new[0], "punctured_MiB": round(pvals / 2 ** 20, 1),
                    "depunctured_MiB": round(dvals / 2 ** 20, 1),
                    "new_ms": round(med(tn), 3), "new_min_ms": round(tn[0], 3), "new_max_ms": round(tn[-1], 3),
                    "a_sibling_on_depunctured_ms": round(med(ta), 3), "a_min_ms": round(ta[0], 3), "a_max_ms": round(ta[-1], 3),
                    "b_gather_then_sibling_ms": round(med(tb), 3), "b_min_ms": round(tb[0], 3), "b_max_ms": round(tb[-1], 3),
                    "gather_alone_ms": round(med(tg), 3),
                    "new_over_a": round(med(tn) / med(ta), 3), "new_over_b": round(med(tn) / med(tb), 3),
                    "ns_per_step": round(med(tn) * 1e6 / (F * T), 4)}
            if name == "frames":
                hwork = torch.empty(max(int(L.cvd_viterbi_frames_workspace_bytes(n, M, T, F, 0)), 16), dtype=torch.uint8,
                                    device=dev)
                pkg._lib.check(L.cvd_viterbi_decode_frames_punctured(code.c, kb, period, ptr(hard), pvals, 2, 0, span, None,
                                                                     F, T, 0, 0, ptr(bits[1]), ptr(frames[1]),
                                                                     ptr(stats[1]), ptr(hwork), stream))
                torch.cuda.synchronize()
                line.update(information_bits=F * (T - M), wrong_bits_soft_punctured=new_wrong,
                            wrong_bits_hard_punctured_on_signs=wrong_bits(bits[1], sent_rows))
                del hwork
            emit(line)
        del pcap, dep, spread, hard, sent, sent_rows, work, llr, bits, frames, stats
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

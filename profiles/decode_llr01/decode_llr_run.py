#!/usr/bin/env python3
"""Device-event timing of the soft-output frame decoder (cvd_viterbi_decode_frames_llr, DESIGN.md
§7.17) on one GPU against cvd_viterbi_decode_frames_soft of the same library (that call's code is
not touched by the soft-output kernel) on the same capture in the same process, the two calls
alternating: F terminated frames of T steps each of (133,171) (random data, m zero tail bits),
BPSK at amplitude A in Gaussian noise of sigma * A, rounded to int8, generated on the device from
a seed.  Per workload F:T, after one warm-up of each call, the median and the minimum of `reps`
event pairs each, and what the output buys: among the frames with a wrong information bit, the
share that lies in the lowest 1% of all frames by `weakest` (ties by frame index).

Prints one JSON line per measurement.

  python profiles/decode_llr01/decode_llr_run.py [--workloads 1048576:128,65536:2048] [--sigma 0.61]
                                                 [--reps 7] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

M, OCT = 6, ("133", "171")


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def terminated_capture(gen, F, T, A, sigma, dev, seed=12345):
    """(int8 values [F * T * n]; the data bits uint8 [F, T], the last m zero)."""
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
    return x.round_().clamp_(-127, 127).to(torch.int8).reshape(-1), u


def pack_lsb(bits):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=bits.device)
    return (bits.reshape(-1, 8) * w).sum(dim=1, dtype=torch.uint8).contiguous()


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

    emit({"device": props.name, "CUs": props.multi_processor_count, "sigma": a.sigma, "amplitude": a.amplitude,
          "reps": a.reps})
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    gen = [[pkg.octal_to_taps(g, M)] for g in OCT]
    n = len(gen)
    code = pkg.Code(gen, M, 1, n)
    for F, T in a.workloads:
        cap, sent = terminated_capture(gen, F, T, a.amplitude, a.sigma, dev)
        nvals, w = cap.numel(), (T + 31) // 32
        assert nvals % 16 == 0
        sent_rows = pack_lsb(torch.nn.functional.pad(sent, (0, 32 * w - T))).reshape(F, 4 * w)
        lwork = int(L.cvd_viterbi_llr_workspace_bytes(n, M, T, F))
        swork = int(L.cvd_viterbi_frames_workspace_bytes(n, M, T, F, 1))
        llr = torch.empty((F, 32 * w), dtype=torch.int16, device=dev)
        lbits, sbits = (torch.empty((F, 4 * w), dtype=torch.uint8, device=dev) for _ in range(2))
        lframes, sframes = (torch.empty((F, 6), dtype=torch.int32, device=dev) for _ in range(2))
        lstats, sstats = (torch.zeros(6, dtype=torch.int64, device=dev) for _ in range(2))
        lwk = torch.empty(lwork, dtype=torch.uint8, device=dev) if lwork else None
        swk = torch.empty(max(swork, 16), dtype=torch.uint8, device=dev)

        def soft_out():
            pkg._lib.check(L.cvd_viterbi_decode_frames_llr(code.c, ptr(cap), nvals, 0, n * T, None, F, T, 0, 0, ptr(llr),
                                                           ptr(lbits), ptr(lframes), ptr(lstats), ptr(lwk), stream))

        def hard_out():
            pkg._lib.check(L.cvd_viterbi_decode_frames_soft(code.c, ptr(cap), nvals, 0, n * T, None, F, T, 0, 0,
                                                            ptr(sbits), ptr(sframes), ptr(sstats), ptr(swk), stream))

        soft_out()
        hard_out()
        torch.cuda.synchronize()
        ls, ss = lstats.cpu().tolist(), sstats.cpu().tolist()
        assert torch.equal(lframes[:, 0], sframes[:, 0]) and torch.equal(lframes[:, 2], sframes[:, 2])
        decided = (llr[:, :T] != 0)
        ub = lambda rows: ((rows.reshape(F, 4 * w, 1) >> torch.arange(8, device=dev, dtype=torch.uint8)) & 1).reshape(F, 32 * w)[:, :T]   # noqa: E731,E501
        assert torch.equal(ub(lbits)[decided], ub(sbits)[decided])
        wrong = (lbits != sent_rows).any(dim=1)
        swrong = (sbits != sent_rows).any(dim=1)
        weakest = lframes[:, 4]
        lowest = torch.argsort(weakest, stable=True)[:max(1, F // 100)]
        caught = int(wrong[lowest].sum())
        lt, st = [], []
        for _ in range(a.reps):                                  # alternating: both see the same neighbours
            lt.append(event_ms(soft_out))
            st.append(event_ms(hard_out))
        lt.sort()
        st.sort()
        l_med, s_med = lt[len(lt) // 2], st[len(st) // 2]
        emit({"code": "133,171", "F": F, "T": T, "decoded": ls[1], "distance": ls[0], "soft_distance": ss[0],
              "zeros": ls[3], "saturated": ls[4], "workspace_MiB": round(lwork / 2 ** 20, 1),
              "frames_soft_workspace_MiB": round(swork / 2 ** 20, 1),
              "llr_ms": round(l_med, 3), "llr_min_ms": round(lt[0], 3), "llr_max_ms": round(lt[-1], 3),
              "frames_soft_ms": round(s_med, 3), "frames_soft_min_ms": round(st[0], 3), "frames_soft_max_ms": round(st[-1], 3),
              "llr_over_frames_soft": round(l_med / s_med, 3), "ns_per_step": round(l_med * 1e6 / (F * T), 4),
              "frames_with_wrong_data": int(wrong.sum()), "frames_soft_frames_with_wrong_data": int(swrong.sum()),
              "lowest_1pct_frames": int(lowest.numel()), "wrong_frames_in_lowest_1pct": caught,
              "share_of_wrong_frames_in_lowest_1pct": round(caught / max(int(wrong.sum()), 1), 4)})
        del cap, sent, sent_rows, llr, lbits, sbits, lframes, sframes, lwk, swk
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

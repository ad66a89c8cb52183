#!/usr/bin/env python3
"""Device-event timing of the list decoder (cvd_viterbi_decode_frames_list) and of
the CRC over its rows (cvd_frames_crc) on one GPU, and what the list buys on CRC-protected frames.

time   F terminated frames of T steps each of (133,171) (random data, m zero tail bits), BPSK at
       amplitude A in Gaussian noise of sigma * A, rounded to int8, generated on the device from a
       seed.  The list call at L = 1, 2, 4, 8 against cvd_viterbi_decode_frames_soft of the same
       library (whose code the list decoder does not touch) on the same capture in the same process,
       the calls alternating after their results were compared (path 0 is that call's): after one
       warm-up of each, the median (min-max) of `reps` event pairs.  Which placement of the
       decisions ran is read off the workspace size (0: the tile in LDS holds a frame).
crc    cvd_frames_crc (crc16-ccitt over T - 22 bits) over the F L rows of the L = 8 result against
       a device copy of the same bytes, and as a share of the list call.
buys   frames of 100 data bits || crc16-ccitt || 6 tail bits.  sigma is swept (on `sweep_frames`
       frames) to where decode_frames_soft loses about one frame in a hundred; there, on
       `buys_frames` frames and for L = 1, 2, 4, 8: frames with crc_ok, among those the frames whose
       chosen bits are what was sent, and the frames that pass the CRC with wrong bits.

Prints one JSON line per measurement.

  python profiles/decode_list01/decode_list_run.py [--workloads 1048576:128,65536:2048] [--sigma 0.61]
                                                   [--reps 7] [--buys-frames 1048576] [--out FILE]
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
LS = (1, 2, 4, 8)


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def med(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def channel(gen, u, A, sigma, g):
    """int8 values [F * T * n] of the input bits u [F, T] encoded from state 0."""
    F, T = u.shape
    n = len(gen)
    sym = torch.zeros((F, T, n), dtype=torch.uint8, device=u.device)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[:, d:, j] ^= u[:, :T - d]                  # u_{t-d}; the encoder starts in state 0
    x = torch.randn((F, T, n), device=u.device, generator=g) * (sigma * A)
    x += (2.0 * sym - 1.0) * A
    return x.round_().clamp_(-127, 127).to(torch.int8).reshape(-1)


def pack_lsb(bits):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=bits.device)
    return (bits.reshape(-1, 8) * w).sum(dim=1, dtype=torch.uint8).contiguous()


def crc16_rows(data):
    """crc16-ccitt (init 0) of the rows of bits data [F, K], first bit first: uint8 [F, 16], MSB first."""
    reg = torch.zeros(data.shape[0], dtype=torch.int32, device=data.device)
    for i in range(data.shape[1]):
        fb = ((reg >> 15) & 1) ^ data[:, i].to(torch.int32)
        reg = ((reg << 1) & 0xFFFF) ^ (fb * 0x1021)
    return ((reg[:, None] >> torch.arange(15, -1, -1, device=data.device)) & 1).to(torch.uint8)


def crc_frames(gen, F, K, A, sigma, dev, seed):
    """(values, the sent rows uint8 [F, 4w]) of F frames of K data bits || crc16 || m zero bits."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    T = K + 16 + M
    u = torch.zeros((F, T), dtype=torch.uint8, device=dev)
    u[:, :K] = torch.randint(0, 2, (F, K), dtype=torch.uint8, device=dev, generator=g)
    u[:, K:K + 16] = crc16_rows(u[:, :K])
    w = (T + 31) // 32
    return channel(gen, u, A, sigma, g), pack_lsb(torch.nn.functional.pad(u, (0, 32 * w - T))).reshape(F, 4 * w), T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="1048576:128,65536:2048",
                    type=lambda s: [tuple(int(x) for x in t.split(":")) for t in s.split(",") if t])
    ap.add_argument("--sigma", type=float, default=0.61)
    ap.add_argument("--amplitude", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--buys-frames", type=int, default=1 << 20)
    ap.add_argument("--sweep-frames", type=int, default=1 << 17)
    ap.add_argument("--sweep", default="0.70,0.75,0.80,0.85,0.90,0.95", type=lambda s: [float(x) for x in s.split(",")])
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

    emit({"device": props.name, "CUs": props.multi_processor_count,
          "clock_MHz": getattr(props, "clock_rate", 0) // 1000, "memory_clock_MHz": getattr(props, "memory_clock_rate", 0) // 1000,
          "sigma": a.sigma, "amplitude": a.amplitude, "reps": a.reps,
          "CVD_LIST_LDS_BYTES": os.environ.get("CVD_LIST_LDS_BYTES"), "CVD_LIST_WAVES": os.environ.get("CVD_LIST_WAVES")})
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    gen = [[pkg.octal_to_taps(g, M)] for g in OCT]
    n = len(gen)
    code = pkg.Code(gen, M, 1, n)

    # ── time ──
    for F, T in a.workloads:
        g = torch.Generator(device=dev)
        g.manual_seed(12345)
        u = torch.randint(0, 2, (F, T), dtype=torch.uint8, device=dev, generator=g)
        u[:, T - M:] = 0
        cap = channel(gen, u, a.amplitude, a.sigma, g)
        del u
        nvals, w = cap.numel(), (T + 31) // 32
        assert nvals % 16 == 0
        swork = int(L.cvd_viterbi_frames_workspace_bytes(n, M, T, F, 1))
        sbits = torch.empty((F, 4 * w), dtype=torch.uint8, device=dev)
        sframes = torch.empty((F, 6), dtype=torch.int32, device=dev)
        sstats = torch.zeros(6, dtype=torch.int64, device=dev)
        swk = torch.empty(max(swork, 16), dtype=torch.uint8, device=dev)

        def best_only():
            pkg._lib.check(L.cvd_viterbi_decode_frames_soft(code.c, ptr(cap), nvals, 0, n * T, None, F, T, 0, 0,
                                                            ptr(sbits), ptr(sframes), ptr(sstats), ptr(swk), stream))

        best_only()
        for Lp in LS:
            lwork = int(L.cvd_viterbi_list_workspace_bytes(n, M, T, F, Lp))
            lbits = torch.empty((F, Lp, 4 * w), dtype=torch.uint8, device=dev)
            lpaths = torch.empty((F, Lp, 3), dtype=torch.int32, device=dev)
            lframes = torch.empty((F, 2), dtype=torch.int32, device=dev)
            lstats = torch.zeros(5, dtype=torch.int64, device=dev)
            lwk = torch.empty(lwork, dtype=torch.uint8, device=dev) if lwork else None

            def listed():
                pkg._lib.check(L.cvd_viterbi_decode_frames_list(code.c, ptr(cap), nvals, 0, n * T, None, F, T, 0, 0, Lp,
                                                                ptr(lbits), ptr(lpaths), ptr(lframes), ptr(lstats),
                                                                ptr(lwk), stream))

            listed()
            torch.cuda.synchronize()
            assert torch.equal(lbits[:, 0], sbits) and torch.equal(lpaths[:, 0, 0], sframes[:, 0])
            assert torch.equal(lpaths[:, 0, 1], sframes[:, 1]) and torch.equal(lpaths[:, 0, 2], sframes[:, 2])
            ls = lstats.cpu().tolist()
            lt, st = [], []
            for _ in range(a.reps):                              # alternating: both see the same neighbours
                lt.append(event_ms(listed))
                st.append(event_ms(best_only))
            lm, sm = med(lt), med(st)
            line = {"measure": "time", "code": "133,171", "F": F, "T": T, "L": Lp, "decoded": ls[1], "paths": ls[3],
                    "workspace_MiB": round(lwork / 2 ** 20, 1), "decisions": "LDS tile" if lwork == 0 else "tiles through d_work",
                    "list": lm, "frames_soft": sm, "list_over_frames_soft": round(lm["ms"] / sm["ms"], 3),
                    "ns_per_step": round(lm["ms"] * 1e6 / (F * T), 4)}
            if Lp == 8:                                          # the CRC over all rows against a copy of them
                value = torch.empty(F * Lp, dtype=torch.int32, device=dev)
                other = torch.empty_like(lbits)

                def crc():
                    pkg._lib.check(L.cvd_frames_crc(ptr(lbits), F * Lp, w, 0, T - 16 - M, 16, 0x1021, 0, ptr(value), stream))

                def copy():
                    other.copy_(lbits)

                crc()
                copy()
                ct, pt = [], []
                for _ in range(a.reps):
                    ct.append(event_ms(crc))
                    pt.append(event_ms(copy))
                cm, pm = med(ct), med(pt)
                emit({"measure": "crc", "F": F, "T": T, "L": Lp, "rows": F * Lp, "words": w, "crc": cm, "device_copy": pm,
                      "crc_over_copy": round(cm["ms"] / pm["ms"], 3), "crc_over_list": round(cm["ms"] / lm["ms"], 4)})
                del value, other
            emit(line)
            del lbits, lpaths, lframes, lwk
        del cap, sbits, sframes, swk

    # ── what it buys ──
    K = 100

    def frame_errors(sigma, F, seed):
        cap, sent, T = crc_frames(gen, F, K, a.amplitude, sigma, dev, seed)
        res = pkg.decode_frames_soft(n, M, gen, cap, T)
        return int((res["bits"] != sent).any(dim=1).sum())

    sweep = []
    for sigma in a.sweep:
        wrong = frame_errors(sigma, a.sweep_frames, 777)
        sweep.append((sigma, wrong / a.sweep_frames))
        emit({"measure": "sweep", "sigma": sigma, "frames": a.sweep_frames, "frames_soft_wrong": wrong,
              "frame_error_rate": round(wrong / a.sweep_frames, 5)})
    sigma = min(sweep, key=lambda p: abs(p[1] - 0.01))[0]
    F = a.buys_frames
    cap, sent, T = crc_frames(gen, F, K, a.amplitude, sigma, dev, 4242)
    for Lp in LS:
        res = pkg.decode_frames_crc(n, M, gen, cap, T, Lp, "crc16-ccitt")
        ok = res["crc_ok"]
        right = (res["chosen_bits"] == sent).all(dim=1)
        emit({"measure": "buys", "sigma": sigma, "frames": F, "T": T, "L": Lp, "crc_ok": int(ok.sum()),
              "crc_ok_and_right": int((ok & right).sum()), "crc_ok_but_wrong": int((ok & ~right).sum()),
              "rescued": res["rescued"], "path0_right": int((res["bits"][:, 0] == sent).all(dim=1).sum())})
        del res
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

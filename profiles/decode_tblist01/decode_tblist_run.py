#!/usr/bin/env python3
"""Device-event timing of the tail-biting list decoder (cvd_viterbi_decode_frames_tailbiting_list,
DESIGN.md §7.20) on one GPU, and what the list buys on tail-biting frames that end in a CRC.

time     F tail-biting frames of T steps each of (133,171,165) (random data, circular encoder), BPSK
         at amplitude A in Gaussian noise of sigma * A, rounded to int8, generated on the device
         from a seed.  The call at L = 1, 2, 4, 8 (T = 40) and L = 4 (T = 128) against
         cvd_viterbi_decode_frames_tailbiting_soft and cvd_viterbi_decode_frames_list (both states
         CVD_FRAME_ANY) of the same library on the same capture in the same process, the three calls
         alternating after path 0 was compared with the tail-biting call's: after one warm-up of
         each, the median (min-max) of `reps` event pairs.  model_ms is (mean laps) x (the list
         call's time): what is left is the all-entries trace and the choice.
quality  LTE-PBCH-shaped frames: 24 data bits || crc16-ccitt, T = 40, tail-biting.  For L = 1, 2, 4,
         8: frames lost (no path passes the CRC, or the chosen bits are not what was sent) and
         frames accepted with wrong bits, for decode_frames_tailbiting_crc and for the workaround
         (decode_frames_tailbiting_soft, then decode_frames_list with both states fixed to path 0's
         end state, frames grouped by that state, and the CRC over its rows).

Prints one JSON line per measurement.

  python profiles/decode_tblist01/decode_tblist_run.py [--frames 1048576] [--sigma 1.1] [--reps 5] [--out FILE]
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

M, OCT = 6, ("133", "171", "165")
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
    """int8 values [F * T * n] of the tail-biting frames u [F, T]: u_{t-d} is taken mod T."""
    F, T = u.shape
    n = len(gen)
    sym = torch.zeros((F, T, n), dtype=torch.uint8, device=u.device)
    for j in range(n):
        for d, tap in enumerate(gen[j][0]):
            if tap:
                sym[:, :, j] ^= torch.roll(u, d, dims=1)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--sigma", type=float, default=1.1)
    ap.add_argument("--amplitude", type=int, default=24)
    ap.add_argument("--reps", type=int, default=5)
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
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")

    emit({"device": props.name, "CUs": props.multi_processor_count, "frames": a.frames, "sigma": a.sigma,
          "amplitude": a.amplitude, "reps": a.reps, "CVD_LIST_LDS_BYTES": os.environ.get("CVD_LIST_LDS_BYTES"),
          "CVD_LIST_WAVES": os.environ.get("CVD_LIST_WAVES")})
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    gen = [[pkg.octal_to_taps(g, M)] for g in OCT]
    n = len(gen)
    code = pkg.Code(gen, M, 1, n)
    F = a.frames

    # ── time ──
    for T, Ls in ((40, LS), (128, (4,))):
        g = torch.Generator(device=dev)
        g.manual_seed(12345)
        u = torch.randint(0, 2, (F, T), dtype=torch.uint8, device=dev, generator=g)
        cap = channel(gen, u, a.amplitude, a.sigma, g)
        del u
        nvals, w = cap.numel(), (T + 31) // 32
        twork = int(L.cvd_viterbi_tailbiting_workspace_bytes(n, M, T, F, 1))
        tbits = torch.empty((F, 4 * w), dtype=torch.uint8, device=dev)
        tframes = torch.empty((F, 8), dtype=torch.int32, device=dev)
        tstats = torch.zeros(9, dtype=torch.int64, device=dev)
        twk = torch.empty(max(twork, 16), dtype=torch.uint8, device=dev)

        def tail():
            pkg._lib.check(L.cvd_viterbi_decode_frames_tailbiting_soft(code.c, ptr(cap), nvals, 0, n * T, None, F, T, 0,
                                                                       ptr(tbits), ptr(tframes), ptr(tstats), ptr(twk),
                                                                       stream))

        tail()
        for Lp in Ls:
            work = int(L.cvd_viterbi_tailbiting_list_workspace_bytes(n, M, T, F, Lp))
            assert work == int(L.cvd_viterbi_list_workspace_bytes(n, M, T, F, Lp))
            bits = torch.empty((F, Lp, 4 * w), dtype=torch.uint8, device=dev)
            paths = torch.empty((F, Lp, 3), dtype=torch.int32, device=dev)
            frames = torch.empty((F, 4), dtype=torch.int32, device=dev)
            lframes = torch.empty((F, 2), dtype=torch.int32, device=dev)
            stats = torch.zeros(8, dtype=torch.int64, device=dev)
            wk = torch.empty(work, dtype=torch.uint8, device=dev) if work else None

            def tblist():
                pkg._lib.check(L.cvd_viterbi_decode_frames_tailbiting_list(code.c, ptr(cap), nvals, 0, n * T, None, F, T, 0,
                                                                           Lp, ptr(bits), ptr(paths), ptr(frames),
                                                                           ptr(stats), ptr(wk), stream))

            def listed():
                pkg._lib.check(L.cvd_viterbi_decode_frames_list(code.c, ptr(cap), nvals, 0, n * T, None, F, T, -1, -1, Lp,
                                                                ptr(bits), ptr(paths), ptr(lframes), ptr(stats), ptr(wk),
                                                                stream))

            listed()
            tblist()                                             # last: the buffers hold its result
            torch.cuda.synchronize()
            assert torch.equal(bits[:, 0], tbits) and torch.equal(paths[:, 0], tframes[:, :3])
            assert torch.equal(frames[:, 1], tframes[:, 3]) and torch.equal(frames[:, 2], tframes[:, 6])
            s = stats.cpu().tolist()
            xt, lt, tt = [], [], []
            for _ in range(a.reps):                              # alternating: all see the same neighbours
                lt.append(event_ms(listed))
                tt.append(event_ms(tail))
                xt.append(event_ms(tblist))
            xm, lm, tm = med(xt), med(lt), med(tt)
            laps = s[7] / s[1]
            emit({"measure": "time", "code": ",".join(OCT), "F": F, "T": T, "L": Lp, "decoded": s[1], "paths": s[3],
                  "status2": s[5], "status3": s[6], "mean_laps": round(laps, 4), "workspace_MiB": round(work / 2 ** 20, 1),
                  "tailbiting_list": xm, "frames_list_any_any": lm, "tailbiting_soft": tm,
                  "model_ms": round(laps * lm["ms"], 3), "over_model": round(xm["ms"] / (laps * lm["ms"]), 3),
                  "over_tailbiting_soft": round(xm["ms"] / tm["ms"], 3), "ns_per_step_lap": round(xm["ms"] * 1e6 / (s[7] * T), 4)})
            del bits, paths, frames, lframes, wk
        del cap, tbits, tframes, twk

    # ── quality ──
    K, T = 24, 40
    g = torch.Generator(device=dev)
    g.manual_seed(4242)
    u = torch.zeros((F, T), dtype=torch.uint8, device=dev)
    u[:, :K] = torch.randint(0, 2, (F, K), dtype=torch.uint8, device=dev, generator=g)
    u[:, K:] = crc16_rows(u[:, :K])
    w = (T + 31) // 32
    sent = pack_lsb(torch.nn.functional.pad(u, (0, 32 * w - T))).reshape(F, 4 * w)
    cap = channel(gen, u, a.amplitude, a.sigma, g)
    del u
    first = pkg.decode_frames_tailbiting_soft(n, M, gen, cap, T)
    state = first["end_states"].to(torch.int64)
    emit({"measure": "quality", "decoder": "tailbiting_soft", "frames": F, "sigma": a.sigma,
          "lost": int((first["bits"] != sent).any(dim=1).sum()), "status2": first["fallback"], "status3": first["open"]})
    for Lp in LS:
        res = pkg.decode_frames_tailbiting_crc(n, M, gen, cap, T, Lp, "crc16-ccitt")
        ok = res["crc_ok"]
        right = (res["chosen_bits"] == sent).all(dim=1)
        emit({"measure": "quality", "decoder": "tailbiting_list", "frames": F, "sigma": a.sigma, "L": Lp,
              "lost": int((~(ok & right)).sum()), "accepted_wrong": int((ok & ~right).sum()), "rescued": res["rescued"],
              "status3_with_candidates": int(((res["status"] == 3) & (res["paths"] > 1)).sum())})
        del res
        lost = wrong = 0
        for s in range(1 << M):                                  # the workaround: both states fixed to path 0's
            idx = torch.nonzero(state == s).reshape(-1)
            if idx.numel() == 0:
                continue
            r = pkg.decode_frames_crc(n, M, gen, cap, T, Lp, "crc16-ccitt", count=K, offsets=idx * (n * T),
                                      start_state=s, end_state=s)
            ok = r["crc_ok"]
            right = (r["chosen_bits"] == sent[idx]).all(dim=1)
            lost += int((~(ok & right)).sum())
            wrong += int((ok & ~right).sum())
            del r
        emit({"measure": "quality", "decoder": "fixed_state_list", "frames": F, "sigma": a.sigma, "L": Lp, "lost": lost,
              "accepted_wrong": wrong})


if __name__ == "__main__":
    main()

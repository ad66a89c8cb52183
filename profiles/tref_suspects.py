#!/usr/bin/env python3
"""How rare the exact T_ref count is behind a one-plane necessary test (csrc/cvd_bitslice.h,
CVD_BS_TREF_FAST).  CPU only.

The received words of the m = 6 pair's H1 and H2 sequences come from the C oracle's stream
generator (oracle/cvd_oracle.c oc_stream: trial t is streams 2t and 2t + 1, the detector's own
trial-id order) at the six headline p; profiles/tref_suspects.cpp runs the header's host step
over them and reports, per candidate plane, the share of lane-steps that pass the test
("suspects"), the share of 64-lane wave-steps with at least one suspect (sequences grouped 64 at
a time, H1 and H2 apart: a unit of the kernel is an all-H1 or an all-H2 wave), and the share of
lane-steps with c > 1.

  python3 profiles/tref_suspects.py [--trials 256] [--steps 4096]

writes profiles/tref_suspects/table.json and table.md.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

P_GRID = [0.01, 0.02, 0.05, 0.10, 0.15, 0.20]
GEN1 = [[[1, 0, 1, 1, 0, 1, 1]], [[1, 1, 1, 1, 0, 0, 1]]]
GEN2 = [[[1, 1, 1, 1, 0, 0, 1]], [[1, 0, 1, 1, 0, 1, 1]]]
SEED = 12345
CANDS = ["plane0", "plane1", "plane2", "plane3", "plane1|2", "plane1|3", "plane2|3"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(HERE, "tref_suspects"))
    args = ap.parse_args()
    from oracle import c_oracle as C
    encs = {"H1": C.Code(GEN1, 6, 1, 2), "H2": C.Code(GEN2, 6, 1, 2)}
    os.makedirs(args.out, exist_ok=True)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tref_suspects")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe,
                               os.path.join(HERE, "tref_suspects.cpp")])
        for p in P_GRID:
            tag = int(C.lib().oc_grid_tag(args.steps, p))
            for h, (hyp, enc) in enumerate(encs.items()):
                w = np.stack([C.stream(enc, args.steps, p, SEED, tag, 2 * t + h) for t in range(args.trials)])
                path = os.path.join(d, "words.bin")
                w.astype(np.uint8).tofile(path)
                out = subprocess.run([exe, path, str(args.trials), str(args.steps)], capture_output=True, text=True,
                                     check=True)
                r = json.loads(out.stdout)
                r.update(p=p, hyp=hyp)
                assert r["missed"] == 0, r   # a c > 1 step that some candidate's test did not pass
                rows.append(r)
                print(p, hyp, {k: r[k]["wave_ge64"] for k in CANDS}, "c>1", r["c_gt1_lane_ge64"], flush=True)
    with open(os.path.join(args.out, "table.json"), "w") as f:
        json.dump({"trials": args.trials, "steps": args.steps, "seed": SEED, "rows": rows}, f, indent=1)
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write(f"Suspects of the one-plane T_ref test: {args.trials} sequences x {args.steps} steps per (p, hypothesis),\n"
                "steps >= 64; lane = share of lane-steps, wave = share of 64-lane wave-steps with a suspect.\n\n")
        f.write("| p | hyp | c > 1 (lane) | " + " | ".join(f"{c.replace('|', '+')} lane / wave" for c in CANDS) + " |\n")
        f.write("|---|---|---|" + "---|" * len(CANDS) + "\n")
        for r in rows:
            f.write(f"| {r['p']} | {r['hyp']} | {r['c_gt1_lane_ge64']:.1e} | " +
                    " | ".join(f"{r[c]['lane_ge64']:.1e} / {r[c]['wave_ge64']:.1e}" for c in CANDS) + " |\n")
        f.write("\nAll steps (the first 64 included), wave share:\n\n")
        f.write("| p | hyp | " + " | ".join(c.replace("|", "+") for c in CANDS) + " |\n|---|---|" + "---|" * len(CANDS) + "\n")
        for r in rows:
            f.write(f"| {r['p']} | {r['hyp']} | " + " | ".join(f"{r[c]['wave']:.1e}" for c in CANDS) + " |\n")
    worst = {c: max(r[c]["wave_ge64"] for r in rows) for c in CANDS}
    print("worst wave share beyond step 64:", worst)


if __name__ == "__main__":
    main()

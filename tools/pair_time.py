#!/usr/bin/env python3
"""Times the paired-code acquisition (gsdr_acq_run_pairs with P pairs) against the plain search
of another build of the library (gsdr_acq_run with 2 P plain code slots and pfa = 0.001), at
N = 16000 x 81 rows and N = 32000 x 81 rows.

The two libraries cannot share a process (gsdr loads one, chosen by GSDR_LIB), so every
measurement is a child process: warm-up calls, then --steps synchronous calls timed with the
host clock (the block's copy to the device and the records' copy back included, the same for
both).  The children alternate, --rounds times per shape: the other build's plain run, this
build's pair run, this build's plain run.  Per shape the tool reports the median of each
round, the spread of the other build's round medians (max - min: its own run-to-run spread,
taken as the margin) and the verdict: pairs not slower than the other build's plain run by
more than that margin.

  GSDR_LIB=<this build> tools/pair_time.py --other <the parent commit's libgsdr.so> --out <file>

Needs a GPU: without one it fails.  Prints one JSON line per shape and writes them to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnss-sdr-new_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(4000000, 16000), (8000000, 32000)]  # 4 ms of Galileo E1 at 4 and 8 Msps
DMAX, DSTEP, ROWS = 10000, 250, 81


def child(args):
    import gsdr
    from gsdr import synth

    assert gsdr.device_count() > 0, "no GPU"
    fs, N, P = args.fs, args.N, args.pairs
    rng = np.random.default_rng(11)
    x = ((rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.5)).astype(np.complex64)
    prns = np.arange(1, P + 1, dtype=np.uint32)
    data = np.stack([synth.gal_e1_sampled(int(p), fs) for p in prns])
    pilot = np.stack([synth.gal_e1_sampled(int(p), fs, pilot=True) for p in prns])
    x = (x + 0.05 * (np.roll(data[0], 2920) + 1j * np.roll(pilot[0], 2920))).astype(np.complex64)
    acq = gsdr.Acquisition(fs, N, DMAX, DSTEP, pfa=0.001, max_prns=2 * P, samples_per_code=float(N),
                           num_doppler_bins=ROWS, fft_size=N, sampled_ms=4, ms_per_code=4)
    if args.child == "pairs":
        acq.set_code_pairs(gsdr.PAIR_SUM_DIFF_J, data, pilot, prns)
        call = lambda: acq.run_pairs(x)  # noqa: E731
    else:
        acq.set_local_codes(np.concatenate([data, pilot]), np.concatenate([prns, prns]))
        call = lambda: acq.run(x)  # noqa: E731
    for _ in range(args.warmup):
        out = call()
    t = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e6)
    q = np.percentile(t, [25, 50, 75])
    r0 = out[0, 0]
    print(json.dumps({"mode": args.child, "lib": gsdr.LIB_PATH, "plan": acq.plan, "q1_us": float("%.5g" % q[0]),
                      "median_us": float("%.5g" % q[1]), "q3_us": float("%.5g" % q[2]),
                      "row0": int(r0["doppler_index"]), "phase0": int(r0["code_phase"])}))
    acq.close()


def run_child(mode, lib, fs, N, args):
    env = dict(os.environ, GSDR_LIB=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--fs", str(fs), "--N", str(N), "--pairs",
           str(args.pairs), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("child failed (%s, %s): %s" % (mode, lib, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default="", help="the library the pair run is compared with (the parent commit's build)")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--fs", type=int, default=0)
    ap.add_argument("--N", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import gsdr

    this = gsdr.LIB_PATH
    assert args.other and os.path.exists(args.other), "--other: the library to compare with"
    rows = []
    for fs, N in SHAPES:
        med = {"other_plain": [], "pairs": [], "this_plain": []}
        last = {}
        for _ in range(args.rounds):
            for key, mode, lib in (("other_plain", "plain", args.other), ("pairs", "pairs", this),
                                   ("this_plain", "plain", this)):
                last[key] = run_child(mode, lib, fs, N, args)
                med[key].append(last[key]["median_us"])
        other = float(np.median(med["other_plain"]))
        spread = float(max(med["other_plain"]) - min(med["other_plain"]))
        pairs = float(np.median(med["pairs"]))
        row = {"fs": fs, "N": N, "rows": ROWS, "pairs": args.pairs, "plain_slots": 2 * args.pairs, "steps": args.steps,
               "rounds": args.rounds, "plan": last["pairs"]["plan"], "round_medians_us": med,
               "other_plain_us": other, "other_spread_us": spread, "pairs_us": pairs,
               "this_plain_us": float(np.median(med["this_plain"])),
               "pairs_minus_other_us": float("%.5g" % (pairs - other)),
               "not_slower_within_spread": bool(pairs <= other + spread),
               # a pair run must find what the plain run over the same slots finds
               "same_winner_cell": (last["pairs"]["row0"], last["pairs"]["phase0"]) ==
                                   (last["this_plain"]["row0"], last["this_plain"]["phase0"])}
        rows.append(row)
        print(json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

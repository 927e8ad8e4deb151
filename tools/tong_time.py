"""Tong cost on the GPU ("Tong"): per-stage device-event times and wall time per call of
gsdr_acq_run_tong with 8 items per call at two workloads (8 PRNs x 41 rows at N = 4000, 4 PRNs x 41
rows at N = 16000) and, for context, gsdr_acq_run of the same 8 blocks.  The two shapes alternate,
the whole sequence runs `rounds` times, and the last line gives every figure's mean and the spread
between the rounds.  No sequence ends (the counter is given room), so every call continues all slots:
the grid is read at the call's first item and written after its last.  One JSON line per
configuration and round.  (profiles/tong/tong_time_per_item_ab.jsonl holds "per_item" lines: the grid kernel
launched once per item, a form this tool timed through a switch that was deleted with it.)

    python tools/tong_time.py [calls per figure, default 50] [rounds, default 3] > out.jsonl
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnss-sdr-new_amd")]
import numpy as np

import gsdr
from gsdr import synth

ITEMS, DMAX, DSTEP = 8, 5000, 250
SHAPES = [(4000, 8), (16000, 4)]  # (N, PRNs)


def stages(acq, call, reps):
    acq.set_profiling(True)
    call()
    acq.read_profile()
    for _ in range(reps):
        call()
    ms, n = acq.read_profile()
    acq.set_profiling(False)
    return [float(m) / reps for m in ms], [int(k) // reps for k in n]


def wall(call, reps):
    for _ in range(3):
        call()
    t = time.perf_counter()
    for _ in range(reps):
        call()
    return (time.perf_counter() - t) / reps * 1e3


def handle(n, nprn, pfa=0.0):
    fs = 1000 * n
    prns = list(range(1, nprn + 1))
    acq = gsdr.Acquisition(fs, n, DMAX, DSTEP, pfa=pfa, max_prns=nprn, max_blocks=ITEMS, samples_per_code=float(n),
                           num_doppler_bins=2 * DMAX // DSTEP + 1, fft_size=n)
    acq.set_local_codes(np.stack([synth.gps_ca_sampled(q, fs) for q in prns]), prns)
    return acq, synth.gps_l1_iq(fs, ITEMS * n, [], seed_offset=3)


def tong(n, nprn, reps, rnd):
    acq, x = handle(n, nprn)
    acq.set_tong(1 << 20, 1 << 30, 1 << 30)
    acq.set_threshold(1.0)
    call = lambda: acq.run_tong(x, nitems=ITEMS)
    st, k = stages(acq, call, reps)
    rec = dict(kind="walking", n=n, prns=nprn, D=acq.num_doppler_bins, items=ITEMS, round=rnd,
               plan=acq.plan["variant"], reuse=acq.spectrum_reuse, stage_ms=st, launches=k, wall_ms=wall(call, reps))
    acq.close()
    print(json.dumps(rec), flush=True)
    return rec


def plain(n, nprn, reps, rnd):
    acq, x = handle(n, nprn, pfa=0.01)
    call = lambda: acq.run(x, nblocks=ITEMS)
    st, k = stages(acq, call, reps)
    rec = dict(kind="plain", n=n, prns=nprn, D=acq.num_doppler_bins, items=ITEMS, round=rnd, plan=acq.plan["variant"],
               reuse=acq.spectrum_reuse, stage_ms=st, launches=k, wall_ms=wall(call, reps))
    acq.close()
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    recs = []
    for rnd in range(rounds):
        for n, nprn in SHAPES:
            recs.append(tong(n, nprn, reps, rnd))
        for n, nprn in SHAPES:
            recs.append(plain(n, nprn, reps, rnd))
    summary = {}
    for kind in ("walking", "plain"):
        for n, _ in SHAPES:
            sel = [r for r in recs if r["kind"] == kind and r["n"] == n]
            if not sel:
                continue
            grid = [r["stage_ms"][1] * 1e3 for r in sel]
            dev = [sum(r["stage_ms"]) * 1e3 for r in sel]
            summary["%s_%d" % (kind, n)] = dict(
                grid_us_mean=round(float(np.mean(grid)), 2), grid_us_spread=round(max(grid) - min(grid), 2),
                device_us_mean=round(float(np.mean(dev)), 2), device_us_spread=round(max(dev) - min(dev), 2),
                wall_us_mean=round(float(np.mean([r["wall_ms"] for r in sel])) * 1e3, 1))
    print(json.dumps(dict(kind="summary", calls=reps, rounds=rounds, figures=summary)), flush=True)

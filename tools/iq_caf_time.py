"""E5a IQ-CAF cost on the GPU ("E5a non-coherent IQ with CAF"): per-stage device-event
times and wall time per call of gsdr_acq_run_iq_caf with 8 items per call, 41 rows, one satellite on
four code slots (2 ms, both components, CAF window 1000 Hz) at N = 32000 and N = 64000, and, as the
baseline, gsdr_acq_run (CFAR) of four PRN slots over the same items on the same build: the same
number of inverse transforms, without the rows kept and summed.  The design this mode's grid kernel
replaces would recompute the two chosen rows, slots + 2 transforms per Doppler row, so the yardstick
is device time below (slots + 2) / slots = 1.5 of the plain run's.  The shapes alternate, the whole
sequence runs `rounds` times, and the last line gives every figure's mean, the spread between the
rounds and the ratio.  One JSON line per configuration and round.

    python tools/iq_caf_time.py [calls per figure, default 20] [rounds, default 3] > out.txt
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

ITEMS, DMAX, DSTEP, SLOTS, WINDOW = 8, 5000, 250, 4, 1000
SIZES = [32000, 64000]


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


def handle(n, pfa):
    fs = 500 * n  # two code periods per item
    acq = gsdr.Acquisition(fs, n, DMAX, DSTEP, pfa=pfa, max_prns=SLOTS, max_blocks=ITEMS, samples_per_code=float(n // 2),
                           num_doppler_bins=2 * DMAX // DSTEP + 1, fft_size=n)
    rng = np.random.default_rng(synth.SEED + n)
    codes = (rng.integers(0, 2, (SLOTS, n)) * 2.0 - 1.0).astype(np.complex64)
    x = ((rng.standard_normal(ITEMS * n) + 1j * rng.standard_normal(ITEMS * n)) * np.sqrt(0.5)).astype(np.complex64)
    return acq, codes, x


def record(kind, n, acq, call, reps, rnd):
    st, k = stages(acq, call, reps)
    rec = dict(kind=kind, n=n, slots=SLOTS, D=acq.num_doppler_bins, items=ITEMS, round=rnd, plan=acq.plan["variant"],
               split=acq.plan["split"], reuse=acq.spectrum_reuse, stage_ms=st, launches=k, wall_ms=wall(call, reps))
    acq.close()
    print(json.dumps(rec), flush=True)
    return rec


def iq_caf(n, reps, rnd):
    acq, codes, x = handle(n, 0.0)
    acq.set_iq_caf(n // 2, 2, True, WINDOW)
    half = np.tile(codes[:2, :n // 2], (1, 2))
    acq.set_iq_codes(half[:1], half[1:], [1])
    return record("iq_caf", n, acq, lambda: acq.run_iq_caf(x, nitems=ITEMS), reps, rnd)


def plain(n, reps, rnd):
    acq, codes, x = handle(n, 0.01)
    acq.set_local_codes(codes, [1, 2, 3, 4])
    return record("plain", n, acq, lambda: acq.run(x, nblocks=ITEMS), reps, rnd)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    recs = []
    for rnd in range(rounds):
        for n in SIZES:
            recs.append(iq_caf(n, reps, rnd))
            recs.append(plain(n, reps, rnd))
    summary = {}
    for n in SIZES:
        dev = {}
        for kind in ("iq_caf", "plain"):
            sel = [r for r in recs if r["kind"] == kind and r["n"] == n]
            tot = [sum(r["stage_ms"]) * 1e3 for r in sel]
            dev[kind] = float(np.mean(tot))
            summary["%s_%d" % (kind, n)] = dict(
                forward_us=round(float(np.mean([r["stage_ms"][0] for r in sel])) * 1e3, 1),
                grid_us=round(float(np.mean([r["stage_ms"][1] for r in sel])) * 1e3, 1),
                device_us_mean=round(dev[kind], 1), device_us_spread=round(max(tot) - min(tot), 1),
                wall_us_mean=round(float(np.mean([r["wall_ms"] for r in sel])) * 1e3, 1))
        summary["ratio_%d" % n] = round(dev["iq_caf"] / dev["plain"], 3)
    print(json.dumps(dict(kind="summary", calls=reps, rounds=rounds, bound=(SLOTS + 2) / SLOTS, figures=summary)),
          flush=True)

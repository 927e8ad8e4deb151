"""QuickSync cost on the GPU ("QuickSync"): per-stage device-event times and wall
time per call of gsdr_acq_run_quicksync at 25 / 8 / 4 Msps against the plain search at the same rate
(8 PRNs, 41 rows), two rounds.  One JSON line per configuration.

    python tools/quicksync_time.py [calls per figure, default 50] [items per call, default 4] > out.jsonl
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

PRNS = list(range(1, 9))


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


def quick(fs, spc, p, dmax, items, reps):
    nf, L = spc // p, p * spc
    D = 2 * dmax // 250 + 1
    acq = gsdr.Acquisition(fs, nf, dmax, 250, max_prns=len(PRNS), max_blocks=items, samples_per_code=float(spc),
                           num_doppler_bins=D, fft_size=nf)
    acq.set_quicksync(p, spc)
    acq.set_quicksync_codes(np.stack([synth.gps_ca_sampled(q, fs) for q in PRNS]), PRNS)
    x = synth.gps_l1_iq(fs, items * L, [], seed_offset=3)
    call = lambda: acq.run_quicksync(x, nitems=items)
    st, n = stages(acq, call, reps)
    w = wall(call, reps)
    rec = dict(kind="quicksync", fs=fs, spc=spc, p=p, nf=nf, D=D, items=items, prns=len(PRNS),
               plan=acq.plan["variant"], reuse=acq.spectrum_reuse, stage_ms=st, launches=n, wall_ms=w,
               ms_of_signal=items * L / fs * 1e3)
    acq.close()
    print(json.dumps(rec), flush=True)


def plain(fs, spc, dmax, blocks, reps):
    D = 2 * dmax // 250 + 1
    acq = gsdr.Acquisition(fs, spc, dmax, 250, pfa=0.01, max_prns=len(PRNS), max_blocks=blocks,
                           samples_per_code=float(spc), num_doppler_bins=D, fft_size=spc)
    acq.set_local_codes(np.stack([synth.gps_ca_sampled(q, fs) for q in PRNS]), PRNS)
    x = synth.gps_l1_iq(fs, blocks * spc, [], seed_offset=3)
    call = lambda: acq.run(x, nblocks=blocks)
    st, n = stages(acq, call, reps)
    w = wall(call, reps)
    rec = dict(kind="plain", fs=fs, spc=spc, D=D, blocks=blocks, prns=len(PRNS), plan=acq.plan["variant"],
               reuse=acq.spectrum_reuse, stage_ms=st, launches=n, wall_ms=w, ms_of_signal=blocks * spc / fs * 1e3)
    acq.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    items = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    for rnd in range(2):
        quick(25000000, 25000, 4, 5000, items, reps)
        quick(8000000, 8000, 2, 5000, items, reps)
        quick(4000000, 4000, 4, 5000, items, reps)
        plain(25000000, 25000, 5000, items, reps)
        plain(8000000, 8000, 5000, items, reps)
        plain(4000000, 4000, 5000, items, reps)

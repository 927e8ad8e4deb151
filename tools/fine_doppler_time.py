#!/usr/bin/env python3
"""Times the fine-Doppler estimate (gsdr_acq_fine_doppler) on the GPU, and beside it the
materialised alternative on the same GPU: torch.fft.fft of the zero-padded 80 N buffer plus
abs().square().argmax().

Per shape (N = 4000 with 1 and 8 requests, N = 25000 with 1 request), after a warm-up:
  kernels_us   device time of the engine's two kernels (HIP events on the handle's stream,
               gsdr_acq_set_profiling: the transform kernel and the finish kernel), median
               and quartiles over --steps calls;
  call_us      host clock around the whole synchronous call (copies of the 10 ms window, the
               code rows and the records included);
  torch_us     HIP events around the wipe-off product, the padded FFT, |.|^2 and argmax of one
               request on the device (input already resident), times the request count for
               the batched shape, since the materialised form runs them one after another.
Needs a GPU: without one it fails.  Prints one JSON line per shape and writes them to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gnss-sdr-new_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gsdr  # noqa: E402
from gsdr import synth  # noqa: E402
from fine_checks import rotate_replica  # noqa: E402  (tests/: the reference's replica alignment)

SHAPES = [(4000000, 4000, 1), (4000000, 4000, 8), (25000000, 25000, 1)]


def quart(v):
    q = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"q1": float("%.4g" % q[0]), "median": float("%.4g" % q[1]), "q3": float("%.4g" % q[2])}


def clocks():
    """The clock state as the tools report it (read only)."""
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True,
                             timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "GPU[0]" in l]
    except Exception as e:  # the tool is optional
        return ["rocm-smi: %s" % e]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    assert gsdr.device_count() > 0 and torch.cuda.is_available(), "no GPU"
    rows = [{"device": torch.cuda.get_device_name(0), "clocks": clocks(), "steps": args.steps, "warmup": args.warmup}]
    print(json.dumps(rows[0]))
    for fs, N, nreq in SHAPES:
        L, M = 10 * N, 80 * N
        # request i searches PRN 1 + i % 3 at code phase 37 i + 5; the first three are the
        # window's satellites at those phases (the sampled replica leads by one sample)
        reqs = [((37 * i + 5) % N, 500.0, i) for i in range(nreq)]
        sats = [synth.Satellite(1 + i, 12.5 * (40 + 16 * i), (37 * i + 4) * 1023.0 / N, 46.0) for i in range(3)]
        x = synth.gps_l1_iq(fs, L, sats, seed_offset=3, t0_samples=2 * N)
        codes = np.stack([synth.gps_ca_sampled(1 + i % 3, fs) for i in range(nreq)])
        acq = gsdr.Acquisition(fs, N, 5000, 250, pfa=0.0, max_prns=1)
        plan = acq.fine_plan
        for _ in range(args.warmup):
            out = acq.fine_doppler(x, codes, reqs)
        acq.set_profiling(True)
        kern, call = [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            acq.fine_doppler(x, codes, reqs)
            call.append((time.perf_counter() - t0) * 1e6)
            ms, n = acq.read_profile()
            assert n[0] == 1 and n[2] == 1, n
            kern.append((ms[0] + ms[2]) * 1e3)
        acq.set_profiling(False)
        # the materialised alternative for one request
        xd = torch.from_numpy(x).cuda()
        cd = torch.from_numpy(np.tile(rotate_replica(codes[0], reqs[0][0]), 10)).cuda()
        buf = torch.zeros(M, dtype=torch.complex64, device="cuda")

        def alt():
            buf[:L] = xd * cd
            return torch.fft.fft(buf).abs().square().argmax()

        for _ in range(args.warmup):
            k = alt()
        torch.cuda.synchronize()
        tt = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            k = alt()
            e1.record()
            e1.synchronize()
            tt.append(e0.elapsed_time(e1) * 1e3 * nreq)
        row = {"fs": fs, "N": N, "nreq": nreq, "fine_plan": plan, "kernels_us": quart(kern), "call_us": quart(call),
               "torch_us": quart(tt), "engine_index0": int(out[0]["index"]), "torch_index0": int(k)}
        rows.append(row)
        print(json.dumps(row))
        acq.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

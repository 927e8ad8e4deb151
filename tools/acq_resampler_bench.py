#!/usr/bin/env python3
"""What the acquisition resampler buys on the 25 Msps GPS L1 C/A grid.

GPS L1 C/A at 25 Msps with the PRN count and Doppler grid of bench.py's C5 GPS grid
(32 PRNs, +-10 kHz in 250 Hz steps), gr_complex items, after an untimed warm-up:

  (a) ms per 1 ms block of run_stream on the 25 Msps ring, N = 25000 -- the only
      way to serve that input without the resampler, so this is the baseline;
  (b) ms per block of Decimator.advance() + run_stream on the decimated ring
      (decimation 10, 49 taps, N = 2500);
  (c) the decimator kernel alone over a 64-block batch, and in the same run a
      device-to-device hipMemcpyAsync of the same input bytes (the kernel reads
      those bytes once and writes a tenth as many).

(a) and (b) run the same schedule: push B blocks from the host, [advance,]
run_stream over those B blocks (synchronous: the results come back to the host);
the push alone is timed too.  The schedules alternate step by step so that clock
and neighbour noise hit them alike.  All times are host clocks around work that
ends in a device synchronise.  Prints one JSON line; --out writes it to a file.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "gnss-sdr-new_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gsdr  # noqa: E402
from gsdr import synth  # noqa: E402

FS, N = 25000000, 25000
PRNS, DMAX, DSTEP = 32, 10000, 250
OPT_FS = 2000000.0  # GPS_L1_CA_OPT_ACQ_FS_SPS


def _hip():
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    return hip


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--blocks", type=int, default=8, help="1 ms blocks per run_stream call (B)")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if gsdr.device_count() < 1:
        raise SystemExit("acq_resampler_bench: no HIP device (a measurement needs the GPU)")
    B, W, K = args.blocks, args.warmup, args.steps
    d, ntaps, latency = gsdr.acq_resampler_plan(FS, OPT_FS)
    fs_d, n_d = FS // d, N // d
    taps = gsdr.firdes_low_pass(1.0, FS, fs_d / 2.1, fs_d / 2.0)
    assert len(taps) == ntaps

    # one step's worth of signal, repeated (the C/A code is periodic in 1 ms blocks)
    sats = synth.random_constellation(12, seed_offset=500, cn0_dbhz=45.0, prns=list(range(1, 13)), max_doppler=4000.0)
    x = synth.gps_l1_iq(FS, B * N, sats, seed_offset=500)
    gsdr.load().gsdr_host_register(ctypes.c_void_p(x.ctypes.data), x.nbytes)
    prns = np.arange(1, PRNS + 1)
    acq_full = gsdr.Acquisition(FS, N, DMAX, DSTEP, pfa=0.01, max_prns=PRNS, max_blocks=B)
    acq_full.set_local_codes(np.stack([synth.gps_ca_sampled(p, FS) for p in prns]), prns)
    acq_dec = gsdr.Acquisition(fs_d, n_d, DMAX, DSTEP, pfa=0.01, max_prns=PRNS, max_blocks=B)
    acq_dec.set_local_codes(np.stack([synth.gps_ca_sampled(p, fs_d) for p in prns]), prns)

    # three rings fed the same pushes: push only, (a), (b)
    r_push, r_a, r_b = (gsdr.Stream(gsdr.ITEM_GR_COMPLEX, 4 * B * N, 2 * B * N) for _ in range(3))
    dec = gsdr.Decimator(r_b, d, taps, 4 * B * n_d, 2 * B * n_d)
    t_push, t_a, t_b = [], [], []
    found_a = found_b = 0
    for step in range(W + K):
        first = step * B * N
        t0 = time.perf_counter()
        r_push.push(x, first)
        r_push.wait_landed(first + B * N)
        t1 = time.perf_counter()
        r_a.push(x, first)
        res_a = acq_full.run_stream(r_a, first, B, stamp0=first + N)
        t2 = time.perf_counter()
        r_b.push(x, first)
        head = dec.advance()
        res_b = acq_dec.run_stream(dec.output, step * B * n_d, B, stamp0=step * B * n_d + n_d)
        t3 = time.perf_counter()
        assert head == (step + 1) * B * n_d
        if step >= W:
            t_push.append((t1 - t0) * 1e3 / B)
            t_a.append((t2 - t1) * 1e3 / B)
            t_b.append((t3 - t2) * 1e3 / B)
            found_a += int(res_a["positive"][:, :12].sum())
            found_b += int(res_b["positive"][:, :12].sum())
    dec.close()
    for r in (r_push, r_a, r_b):
        r.close()

    # (c) the kernel alone over 64 blocks, against a D2D copy of the same bytes
    NB = 64
    items = NB * N
    src = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, 2 * (NB + 1) * N, (NB + 1) * N)
    dk = gsdr.Decimator(src, d, taps, 4 * NB * n_d, NB * n_d)
    hip = _hip()
    a_dev, b_dev = ctypes.c_void_p(), ctypes.c_void_p()
    nbytes = items * 8
    assert hip.hipMalloc(ctypes.byref(a_dev), nbytes) == 0 and hip.hipMalloc(ctypes.byref(b_dev), nbytes) == 0
    hip.hipMemset(a_dev, 0, nbytes)
    hip.hipMemset(b_dev, 0, nbytes)
    t_k, t_c = [], []
    pushed = 0
    for rep in range(args.kernel_reps + 3):
        for _ in range(NB // B):
            src.push(x, pushed)
            pushed += B * N
        src.wait_landed(pushed)
        t0 = time.perf_counter()
        head = dk.advance()
        dk.output.window(head - 1, 1)  # waits for the passes
        t1 = time.perf_counter()
        hip.hipMemcpyAsync(b_dev, a_dev, nbytes, 3, None)  # hipMemcpyDeviceToDevice
        hip.hipStreamSynchronize(None)
        t2 = time.perf_counter()
        if rep >= 3:
            t_k.append((t1 - t0) * 1e3)
            t_c.append((t2 - t1) * 1e3)
    dk.close()
    src.close()
    hip.hipFree(a_dev)
    hip.hipFree(b_dev)
    gsdr.load().gsdr_host_unregister(ctypes.c_void_p(x.ctypes.data))

    a_ms, b_ms = statistics.median(t_a), statistics.median(t_b)
    k_ms, c_ms = statistics.median(t_k), statistics.median(t_c)
    out = {
        "tool": "tools/acq_resampler_bench.py",
        "workload": "GPS L1 C/A, %d Msps gr_complex, %d PRNs x %d Doppler bins, %d blocks per call, %d timed steps after "
                    "%d warm-up" % (FS // 1000000, PRNS, acq_full.num_doppler_bins, B, K, W),
        "resampler": {"decimation": d, "ntaps": ntaps, "latency": latency, "fs_decimated": fs_d, "fft_size": n_d},
        "timing": "host clock around push + [advance +] run_stream (synchronous), per 1 ms block",
        "push_only_ms_per_block": _stats(t_push),
        "a_full_rate_ms_per_block": _stats(t_a),
        "b_resampled_ms_per_block": _stats(t_b),
        "a_over_b": round(a_ms / b_ms, 3),
        "positives_of_the_12_satellites": {"a": found_a, "b": found_b, "of": 12 * B * K},
        "c_kernel_64_blocks": {
            "input_bytes": nbytes, "output_bytes": nbytes // d,
            "advance_ms": _stats(t_k), "d2d_memcpy_ms": _stats(t_c),
            "kernel_over_copy": round(k_ms / c_ms, 3),
            "input_gb_per_s": round(nbytes / (k_ms * 1e-3) / 1e9, 1),
            "note": "host clock around advance() + wait and around hipMemcpyAsync + synchronise: both include one "
                    "launch and one wait",
        },
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""Per-call kernel time of the tracking loop, Kalman against DLL/PLL ("Kalman loop"):
gsdr_trk_read_profile's device-event time of one launch over `calls` general_work calls, divided by
the calls, for GPS L1 C/A pools at the C2 tracking shape (4 Msps, 8 channels) and a C5 shape (25 Msps,
8 channels, the streamed correlation).  Both loops track the same satellites on the same input from
the same start; a launch of each alternates, the whole sequence runs `rounds` times, and the last line
gives each figure's median and the spread between the rounds.  One JSON line per launch.

    python tools/kf_time.py [calls per launch, default 200] [rounds, default 7] > out.jsonl
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gnss-sdr-new_amd")]
import numpy as np

import gsdr
from gsdr import synth

SHAPES = [("C2", 4.0e6, 8), ("C5", 25.0e6, 8)]  # (name, fs, channels)


def pool(fs, nch, kf, sats, iq, calls):
    c = gsdr.trk_conf_default()
    c["fs_in"], c["max_channels"], c["pull_in_time_s"] = fs, nch, 0
    t = gsdr.Tracking(c)
    if kf:
        t.set_kf()
    vl = int(round(fs / 1000))
    for ch, s in enumerate(sats):
        tau = s.code_delay_chips / (1.023e6 * (1 + s.doppler_hz / 1.57542e9)) * fs
        t.start(ch, s.prn, synth.gps_ca_chips(s.prn), float(round(tau) % vl), float(250 * round(s.doppler_hz / 250)), 0, 0)
    t.save_state(0)
    t.run(iq, 0, calls)  # warm: the input is on the device after this
    return t


def launch_us(t, iq, calls):
    t.restore_state(0)
    t.set_profiling(True)
    _, n = t.run(iq, 0, calls)
    ms, launches = t.read_profile()
    t.set_profiling(False)
    assert launches == 1 and int(n.min()) == calls, (launches, n)
    return ms * 1e3 / calls


if __name__ == "__main__":
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    figures = {}
    for name, fs, nch in SHAPES:
        sats = synth.random_constellation(nch, seed_offset=2, cn0_dbhz=47.0)
        iq = synth.gps_l1_iq(fs, int((calls + 3) * fs / 1000), sats, seed_offset=2)
        loops = {"dll_pll": pool(fs, nch, False, sats, iq, calls), "kf": pool(fs, nch, True, sats, iq, calls)}
        got = {k: [] for k in loops}
        for rnd in range(rounds):
            for k, t in loops.items():
                us = launch_us(t, iq, calls)
                got[k].append(us)
                print(json.dumps(dict(shape=name, fs=fs, channels=nch, loop=k, round=rnd, calls=calls, us_per_call=us)),
                      flush=True)
        for k, v in got.items():
            figures["%s_%s" % (name, k)] = dict(us_median=round(float(np.median(v)), 3),
                                               us_spread=round(max(v) - min(v), 3))
        for t in loops.values():
            t.close()
    print(json.dumps(dict(kind="summary", calls=calls, rounds=rounds, figures=figures)), flush=True)

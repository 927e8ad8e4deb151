"""tests/trk_restatement.py pinned (no GPU).

1. Agreement with the C oracle (oracle/trk_oracle.c) on the signals both know: the
   restatement replays the records of a free-running oracle.trk.Channel (the oracle's own
   correlator outputs, call by call) through pull-in, bit synchronisation and state 4:
   1.3 s at 2 Msps, the trk_checks.py scenario.  States, flags and the emitted prompts
   agree exactly and every float field within the tolerances trk_checks._replay_check
   uses between two float evaluations of the loop (worst distances: DESIGN.md).
2. The restatement free-running on Galileo E5a and GPS L5, pilot and data tracking, at
   4 Msps (and E5a pilot at 5 Msps): the scenarios of test_gpu_trk_wideband.py checked on
   the CPU first.
"""
import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import trk

import trk_restatement
import trk_wideband_checks as wb
from trk_checks import FS, SAT, SIGNAL_S, _acq, _conf, _conf_sig, _replay_check

N_CALLS = {0: 1290, 1: 320, 2: 1290}


def _oracle_scenario(name):
    n = int(SIGNAL_S * FS)
    if name == "gps":
        delay, dop = _acq(SAT, FS)
        return _conf(FS), synth.gps_l1_iq(FS, n, [SAT], seed_offset=5), synth.gps_ca_chips(SAT.prn), None, delay, dop, SAT.prn
    if name.startswith("gal"):
        pilot = name == "gal_pilot"
        sat = synth.GalileoSatellite(11, 1234.5, 1000.3, 50.0, 0.7)
        tau = sat.code_delay_chips / (1.023e6 * (1 + sat.doppler_hz / 1.57542e9)) * FS
        code = synth.gal_e1_sinboc11(11, pilot=pilot)
        return (_conf_sig(FS, gsdr.SIGNAL_GAL_1B, 1, int(pilot)), synth.gal_e1_iq(FS, n, [sat], seed_offset=5), code,
                synth.gal_e1_sinboc11(11) if pilot else None, float(round(tau) % 8000), 1250.0, 11)
    prn = int(name[3:])
    s = synth.Satellite(prn, -2262.3, 500.2, 45.0, 0.3)
    tau = s.code_delay_chips / (2.046e6 * (1 + s.doppler_hz / 1.561098e9)) * FS
    return (_conf_sig(FS, gsdr.SIGNAL_BDS_B1), synth.bds_b1i_iq(FS, n, [s], seed_offset=7), synth.bds_b1i_chips(prn), None,
            float(round(tau) % 2000), -2250.0, prn)


@pytest.mark.parametrize("name", ["gps", "gal_pilot", "gal_data", "bds14", "bds3"])
def test_restatement_replays_the_oracle(name):
    conf, iq, code, dcode, delay, dop, prn = _oracle_scenario(name)
    oc = conf[0:1].view(trk.TRK_CONF_DTYPE)
    free = trk.Channel(oc)
    first = free.start(code, delay, dop, 0, 0, prn=prn, data_code=dcode)
    recs, _ = free.run(iq, 0, first, 2000)
    assert recs["state"][-1] == 4 and np.count_nonzero(recs["flags"] & gsdr.TRK_F_BIT_SYNC) == 1, name
    assert {2, 4} <= set(np.unique(recs["state"]).tolist())
    ch = trk_restatement.Channel(oc)
    assert ch.start(code, delay, dop, 0, 0, prn=prn, data_code=dcode) == first
    o = _replay_check(recs, ch, name)
    for f in ("carrier_doppler_hz", "code_freq_chips", "rem_code_phase_samples", "acc_carrier_phase_rad", "cn0_db_hz",
              "carrier_lock_test", "evm"):
        print("%s %s %.3e" % (name, f, np.max(np.abs(recs[f] - o[f]))))


@pytest.mark.parametrize("system,pilot,fs", [k + (4.0e6,) for k in wb.CASES] + [("5X", 1, 5.0e6)])
def test_restatement_free_run_on_wideband_signals(system, pilot, fs):
    c = wb.case(system, pilot, fs)
    ch, first = c.restatement()
    assert first == c.first
    recs, _ = ch.run(c.iq, 0, first, 1400)
    assert len(recs) >= 1290
    wb.check_locked_run(recs, c)
    # the replay of its own records reproduces the emitted prompts and flags
    rep, _ = c.restatement()
    again = rep.replay(recs)
    np.testing.assert_array_equal(again["prompt_i"], recs["prompt_i"])
    np.testing.assert_array_equal(again["flags"], recs["flags"])

"""The Kalman-loop restatement (kf_restatement.KfChannel) pinned without a GPU.

The reference's kf_tracking cannot be built here and ships no captured numbers, so
KfChannel is pinned by construction: its matrices against literals written out below,
one run_Kf step against an independent evaluation, the Q accumulation of the narrow
update against the sum written out; then its free run on the project's scenarios.
"""
import functools
import math

import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import trk

import kf_restatement as kr
from trk_checks import FS, NITEMS, SAT, _conf, scenario_input
from test_trk_restatement import _oracle_scenario

PI = 3.1415926535898
BETA = 1.023e6 / 1.57542e9
TRUE_DOPPLER = SAT.doppler_hz
GPS_CALLS = 1298


def _gps_channel(extend=1, variant="ref"):
    c = _conf(FS)
    c["extend_correlation_symbols"] = extend
    _, _, (prn, delay, dop) = scenario_input("signal")
    ch = kr.KfChannel(c[0:1].view(trk.TRK_CONF_DTYPE), variant=variant)
    first = ch.start(synth.gps_ca_chips(prn), delay, dop, 0, NITEMS)
    return ch, first, dop


def test_matrices_after_start():
    ch, _, dop = _gps_channel()
    Ti = 0.001
    F = [[1.0, 0.0, BETA * 1e-3, BETA * 1e-6 / 2.0],
         [0.0, 1.0, 2.0 * PI * 1e-3, PI * 1e-6],
         [0.0, 0.0, 1.0, 1e-3],
         [0.0, 0.0, 0.0, 1.0]]
    H = [[1.0, 0.0, -BETA * 1e-3 / 2.0, BETA * 1e-6 / 6.0],
         [0.0, 1.0, -PI * 1e-3, PI * 1e-6 / 3.0]]
    assert ch.corr_time == Ti
    np.testing.assert_allclose(ch.F, F, rtol=1e-15, atol=0)
    np.testing.assert_allclose(ch.H, H, rtol=1e-15, atol=0)
    # the entries as numbers: beta = 6.4935e-4 chips per carrier cycle
    np.testing.assert_allclose(ch.F[0, 2:], [6.493506493506494e-07, 3.246753246753247e-10], rtol=1e-12)
    np.testing.assert_allclose(ch.F[1, 2:], [6.2831853071796e-03, 3.1415926535898e-06], rtol=1e-13)
    np.testing.assert_allclose(ch.H[:, 2:], [[-3.246753246753247e-07, 1.0822510822510823e-10],
                                            [-3.1415926535898e-03, 1.0471975511966e-06]], rtol=1e-12)
    np.testing.assert_allclose(ch.R, np.diag([0.04, 0.09]), rtol=1e-15)
    np.testing.assert_allclose(ch.Q, np.diag([0.0225, 0.0625, 0.36, 1e-4]), rtol=1e-15)
    np.testing.assert_allclose(ch.Pk, np.diag([0.25, 0.49, 25.0, 1.0]), rtol=1e-15)
    np.testing.assert_array_equal(ch.xk, [0.0, 0.0, dop, 0.0])


def _textbook_step(F, H, Q, R, x, P, z):
    """The textbook filter, element by element in Python floats, S solved not inverted."""
    n = 4
    xm = [sum(F[i][k] * x[k] for k in range(n)) for i in range(n)]
    FP = [[sum(F[i][k] * P[k][j] for k in range(n)) for j in range(n)] for i in range(n)]
    Pm = np.array([[sum(FP[i][k] * F[j][k] for k in reversed(range(n))) + Q[i][j] for j in range(n)] for i in range(n)])
    HP = H @ Pm
    S = HP @ H.T + R
    K = np.linalg.solve(S, HP).T  # K = Pm H^T S^-1 with S and Pm symmetric
    innov = z
    xn = np.array(xm) + K @ innov
    Pn = Pm - K @ S @ K.T
    return xn, Pn


def test_one_step_against_independent_evaluation():
    ch, _, dop = _gps_channel()
    ch.state = 2
    ch.E, ch.P, ch.L = [kr.f32(810.0), kr.f32(95.0)], [kr.f32(1500.0), kr.f32(240.0)], [kr.f32(700.0), kr.f32(80.0)]
    ph = math.atan(240.0 / 1500.0) / (2.0 * PI)
    pe, pl = math.hypot(810.0, 95.0), math.hypot(700.0, 80.0)
    code = (1.0 - 0.25) * (pe - pl) / (pe + pl)
    z = np.array([code, ph * 2.0 * PI])
    x0, P0 = ch.xk.copy(), ch.Pk.copy()
    xt, Pt = _textbook_step(ch.F, ch.H, ch.Q, ch.R, x0, P0, z)
    rem0 = ch.rem_code_samples
    ch._run_dll_pll()
    assert abs(ch.errs[0] - ph) <= 1e-8 and abs(ch.errs[2] - code) <= 1e-7  # float atan / hypot in the restatement
    xs, Ps = kr.kf_step(ch.F, ch.H, ch.Q, ch.R, x0, P0, np.array([ch.errs[2], ch.errs[0] * 2.0 * PI]), "solve")
    xt, Pt = _textbook_step(ch.F, ch.H, ch.Q, ch.R, x0, P0, np.array([ch.errs[2], ch.errs[0] * 2.0 * PI]))
    for xo, Po in ((xs, Ps), (xt, Pt)):
        np.testing.assert_allclose(ch.Pk, Po, rtol=0, atol=1e-13 * np.abs(Po).max())
        np.testing.assert_allclose(ch.xk[1:], xo[1:], rtol=0, atol=1e-13 * np.abs(xo).max())
        assert abs(ch.errs[3] - xo[0]) <= 1e-15
    assert ch.xk[0] == 0.0
    assert ch.carrier_doppler == ch.xk[2] and ch.rem_carr == kr.f32(ch.xk[1])
    assert ch.code_freq == 1.023e6 + ch.xk[2] * 1.023e6 / 1.57542e9
    assert ch.rem_code_samples == rem0 + FS * ch.errs[3] / ch.code_freq
    assert ch.errs[1] == float(kr.f32(ch.xk[2]))


@pytest.mark.parametrize("extend", [1, 4])
def test_narrow_update_accumulates_q(extend):
    ch, _, _ = _gps_channel(extend)
    F, Q0 = ch.F.copy(), ch.Q.copy()
    ch.cn0, ch.corr_time = 44.0, float(kr.f32(kr.f32(extend) * kr.f32(0.001)))
    ch._update_kf_narrow()
    want = np.zeros((4, 4))
    Fn = np.eye(4)
    for _ in range(extend):
        Fn = F @ Fn
        want += Fn @ Q0 @ Fn.T  # sum_{n=1..extend} F^n Q (F^n)^T
    np.testing.assert_allclose(ch.Q, want, rtol=1e-13, atol=0)
    Fw, Hw = kr.model(BETA, ch.corr_time)
    np.testing.assert_array_equal(ch.F, Fw)
    np.testing.assert_array_equal(ch.H, Hw)
    lt = 10.0 ** 4.4 * ch.corr_time
    np.testing.assert_allclose(np.diag(ch.R), [(0.25 + 0.25 / 0.75 / (2 * lt)) / lt, (1 + 1 / (2 * lt)) / (2 * lt)],
                               rtol=1e-13)


@functools.lru_cache(maxsize=None)
def gps_free_run(extend):
    """(records, channel, first sample) of the free-running restatement; shared, read-only."""
    iq, _, _ = scenario_input("signal")
    ch, first, _ = _gps_channel(extend)
    recs, _ = ch.run(iq, 0, first, GPS_CALLS)
    recs.setflags(write=False)
    return recs, ch, first


# the call of the bit synchronisation and of the first output, per extend_correlation_symbols
GPS_SHAPE = {1: (1158, 1178), 4: (1158, 1178)}


@pytest.mark.parametrize("extend", [1, 4])
def test_gps_free_run(extend):
    recs, ch, _ = gps_free_run(extend)
    sync_call, first_out = GPS_SHAPE[extend]
    assert len(recs) == GPS_CALLS
    assert not np.any(recs["flags"] & gsdr.TRK_F_LOSS_OF_LOCK)
    np.testing.assert_array_equal(np.nonzero(recs["flags"] & gsdr.TRK_F_BIT_SYNC)[0], [sync_call])
    assert ch.state == 4  # the run ends in state 4 (the last record of extend 4 is the state-3 call before it)
    assert (3 in recs["state"]) == (extend > 1)
    outs = np.nonzero(recs["flags"] & gsdr.TRK_F_VALID_OUTPUT)[0]
    assert outs[0] == first_out and np.all(np.diff(outs) == 20)
    s4 = recs["state"] == 4
    dop = recs["carrier_doppler_hz"]
    # within 0.2 Hz rms of the truth once the 15.5 Hz offset of the acquisition grid has decayed: over the
    # settled wide-tracking calls, 300 up to the synchronisation, which are most of the run (0.19 Hz).  In
    # state 4 R is re-derived from the C/N0 and smaller than the configured one, the gain is higher and
    # the estimate noisier with 1 ms integration: 0.275 Hz rms for extend 1, 0.15 Hz for extend 4.
    rms2 = np.sqrt(np.mean((dop[300:sync_call] - TRUE_DOPPLER) ** 2))
    rms4 = np.sqrt(np.mean((dop[s4] - TRUE_DOPPLER) ** 2))
    print("extend %d: Doppler rms %.3f Hz over calls 300..sync, %.3f Hz over state 4, state-4 mean %.3f" %
          (extend, rms2, rms4, dop[s4].mean()))
    assert rms2 <= 0.2
    if extend > 1:
        assert rms4 <= 0.2
    assert abs(dop[s4].mean() - TRUE_DOPPLER) <= 1.0
    assert np.all(recs["evm"] == 0.0) and np.all(recs["carrier_rate"] == 0.0) and np.all(recs["code_rate"] == 0.0)


def _state4_step_from_scratch(make, recs, k):
    """Call k of a run (a state-4 call) rebuilt outside the restatement: the channel replays the
    records before it, then update_kf_cn0's H and R (:938-955) and run_Kf's step are written out here
    from the record's own C/N0 and discriminator outputs.  Returns (Doppler predicted, |z1|)."""
    ch = make()
    ch.replay(recs[:k])
    Ti, spc = ch.corr_time, float(ch.spc)
    beta = ch.chip_rate / ch.carrier_hz
    F = np.array([[1, 0, beta * Ti, beta * Ti * Ti / 2], [0, 1, 2 * PI * Ti, PI * Ti * Ti], [0, 0, 1, Ti], [0, 0, 0, 1.0]])
    H = np.array([[1, 0, -beta * Ti / 2, beta * Ti * Ti / 6], [0, 1, -PI * Ti, PI * Ti * Ti / 3]])
    lt = 10.0 ** (float(recs["cn0_db_hz"][k]) / 10.0) * Ti
    R = np.diag([(spc + spc / (1 - spc) / (2 * lt)) / lt, (1 + 1 / (2 * lt)) / (2 * lt)])
    z = np.array([float(recs["code_error_chips"][k]), float(recs["carr_phase_error_hz"][k]) * 2.0 * PI])
    x, _ = _textbook_step(F, H, ch.Q, R, ch.xk.copy(), ch.Pk.copy(), z)
    return x[2], abs(z[1])


@pytest.mark.parametrize("extend", [1, 4])
def test_state4_step_rebuilds_h_and_r_from_cn0(extend):
    """update_kf_cn0 on a run: the Doppler of two state-4 calls from a step written out in the test
    (the discriminators from the records are floats: 1e-5 Hz)."""
    recs, _, _ = gps_free_run(extend)
    s4 = np.nonzero(recs["state"] == 4)[0]
    for k in (int(s4[0]), int(s4[-1])):
        want, _ = _state4_step_from_scratch(lambda: _gps_channel(extend)[0], recs, k)
        assert abs(recs["carrier_doppler_hz"][k] - want) <= 1e-5, (k, recs["carrier_doppler_hz"][k], want)


GAL_CALLS = 320


def _gal_channel():
    conf, _, code, dcode, delay, dop, prn = _oracle_scenario("gal_pilot")
    ch = kr.KfChannel(conf[0:1].view(trk.TRK_CONF_DTYPE))
    return ch, ch.start(code, delay, dop, 0, 0, prn=prn, data_code=dcode)


@functools.lru_cache(maxsize=None)
def gal_free_run(calls=GAL_CALLS):
    """The gal_pilot scenario of test_trk_restatement.py; more than 320 calls on the same satellite and
    noise seed generated for longer."""
    _, iq, _, _, _, _, _ = _oracle_scenario("gal_pilot")
    if calls > GAL_CALLS:
        sat = synth.GalileoSatellite(11, 1234.5, 1000.3, 50.0, 0.7)
        iq = synth.gal_e1_iq(FS, int(2.6 * FS), [sat], seed_offset=5)  # 650 calls
    ch, first = _gal_channel()
    recs, _ = ch.run(iq, 0, first, calls)
    recs.setflags(write=False)
    return recs, ch, first


def test_gal_pilot_free_run():
    """The E1 pilot run the same way as the GPS runs: the loop holds lock at default values, finds the
    secondary code at call 273 and stays in state 4; the mean Doppler over the state-4 calls is within
    1 Hz of the truth.  The scenario's 1.3 s leave 46 calls in state 4, which begin with a step of the
    Doppler estimate by -6.5 Hz, so this run is 640 calls (2.56 s) of the same satellite.

    The step is the reference's: the two-quadrant (Costas) discriminator of state 2 locks at either
    of two phases half a cycle apart.  Here it holds the one at which acquire_secondary (:997-1034)
    finds the prompt negative on the secondary chip '0', which that function counts as a match and
    reports without the 180 degree flag; save_correlation_results (:1320-1330) adds those prompts
    unchanged, d_cloop is false from then on, and run_Kf's four-quadrant discriminator (:1140) reads
    -0.49 cycles where the two-quadrant one read 0: an innovation of -pi rad into the never wrapped
    x(1), which the gain K(2,1) of about 2 Hz/rad turns into -6.5 Hz of x(2).  Nothing in run_Kf looks
    at the flag.  The step is checked below against a filter step written out in the test."""
    recs, ch, _ = gal_free_run(640)
    assert len(recs) == 640 and ch.state == 4
    assert not np.any(recs["flags"] & gsdr.TRK_F_LOSS_OF_LOCK)
    np.testing.assert_array_equal(np.nonzero(recs["flags"] & gsdr.TRK_F_BIT_SYNC)[0], [273])
    assert set(np.unique(recs["state"]).tolist()) == {2, 4} and np.all(recs["state"][274:] == 4)
    outs = np.nonzero(recs["flags"] & gsdr.TRK_F_VALID_OUTPUT)[0]
    np.testing.assert_array_equal(outs, np.arange(274, 640))
    dop = recs["carrier_doppler_hz"]
    s4 = recs["state"] == 4
    print("gal_pilot: state-4 Doppler mean %.3f rms %.3f; step at the hand-over %.3f Hz" %
          (dop[s4].mean(), np.sqrt(np.mean((dop[s4] - 1234.5) ** 2)), dop[274] - dop[273]))
    assert abs(dop[s4].mean() - 1234.5) <= 1.0
    # the hand-over: no 180 degree flag, a discriminator of half a cycle, and the Doppler the step gives
    assert not np.any(recs["flags"] & gsdr.TRK_F_PLL_180)
    assert abs(abs(float(recs["carr_phase_error_hz"][274])) - 0.5) <= 0.02
    assert abs(float(recs["carr_phase_error_hz"][273])) <= 0.05
    want, z1 = _state4_step_from_scratch(lambda: _gal_channel()[0], recs, 274)
    assert z1 >= 3.0 and abs(dop[274] - want) <= 1e-5, (dop[274], want, z1)
    assert -8.0 <= dop[274] - dop[273] <= -5.0

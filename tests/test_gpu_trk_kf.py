"""The Kalman tracking loop (Tracking.set_kf) on the GPU against kf_restatement.KfChannel.

1. loop parity: open-loop taps, the restatement replayed on the GPU's taps (the bars of
   trk_checks._replay_check), the locked shape of the CPU free run;
2. the filter's x and P after the run against the replay's, within 100 times the distance
   between two CPU evaluations of the same replay (KfChannel as committed and its
   `solve` variant: other association orders, np.linalg.solve for the 2x2 inverse) --
   the device sums its sparse products in the restatement's order;
3. channels of one pool do not mix; 4. save / restore carries the filter; 5. a forced
   loss drops the call's filter step and a new start re-initialises the filter;
6. the ring path; 7. the refusals of gsdr_trk_set_kf / gsdr_trk_get_kf_state; 8. the host adapter
   (kf_tracking_selftest) against the C ABI records; and the E5a pilot on the compact replicas.
"""
import functools

import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import trk

import kf_restatement as kr
import trk_checks as tc
from trk_checks import _open_loop_sig, _open_loop_taps, _replay_check
from test_kf_restatement import GPS_CALLS, GPS_SHAPE, gal_free_run, gps_free_run
from test_trk_restatement import _oracle_scenario

pytestmark = pytest.mark.gpu

FS = tc.FS
LOST = gsdr.TRK_F_LOSS_OF_LOCK


def _gps_conf(extend=1, nch=1):
    c = tc._conf(FS, nch)
    c["extend_correlation_symbols"] = extend
    return c


def _gps_kf(conf, variant="ref"):
    _, _, (prn, delay, dop) = tc.scenario_input("signal")
    ch = kr.KfChannel(conf[0:1].view(trk.TRK_CONF_DTYPE), variant=variant)
    return ch, ch.start(synth.gps_ca_chips(prn), delay, dop, 0, tc.NITEMS)


@functools.lru_cache(maxsize=None)
def _gps_gpu_run(extend):
    """One Kalman channel on the scenario signal: (records, x, P, first sample)."""
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    t = gsdr.Tracking(_gps_conf(extend))
    t.set_kf()
    first = t.start(0, prn, synth.gps_ca_chips(prn), delay, dop, 0, tc.NITEMS)
    rec, n = t.run(iq, 0, GPS_CALLS)
    g = rec[0][:n[0]].copy()
    x, P = t.kf_state(0)
    t.close()
    g.setflags(write=False)
    return g, x, P, first


def _state_bar(ref, alt):
    """The largest difference between two CPU evaluations, relative to max|x| and max|P|."""
    dx = np.max(np.abs(ref.xk - alt.xk)) / np.max(np.abs(ref.xk))
    dP = np.max(np.abs(ref.Pk - alt.Pk)) / np.max(np.abs(ref.Pk))
    return dx, dP


def _state_distances(x, P, g, make, tag):
    """(GPU x distance, its bar, GPU P distance, its bar): the bars are 100 times the distance
    between the two CPU evaluations of the replay."""
    ref, alt = make("ref"), make("solve")
    ref.replay(g)
    alt.replay(g)
    bx, bP = _state_bar(ref, alt)
    dx = np.max(np.abs(x - ref.xk)) / np.max(np.abs(ref.xk))
    dP = np.max(np.abs(P - ref.Pk)) / np.max(np.abs(ref.Pk))
    print("%s: CPU ref vs solve x %.3e P %.3e; GPU vs ref x %.3e P %.3e" % (tag, bx, bP, dx, dP))
    return dx, 100 * bx, dP, 100 * bP


@pytest.mark.parametrize("extend", [1, 4])
def test_gps_loop_parity_and_covariance(extend):
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    code = synth.gps_ca_chips(prn)
    g, x, P, first = _gps_gpu_run(extend)
    conf = _gps_conf(extend)
    rep, first_o = _gps_kf(conf)
    assert first == first_o and len(g) == GPS_CALLS
    if extend > 1:
        assert _open_loop_sig(g, iq, code, None, FS, dop, [-0.25, 0, 0.25], 1, 1.023e6, 2000, 1, [-0.15, 0, 0.15]) <= 1e-4
    else:
        assert _open_loop_taps(g, iq, code, FS, dop) <= 1e-4
    _replay_check(g, rep, "kf gps extend %d" % extend)
    # the shape of the CPU free run, which locked
    free, _, _ = gps_free_run(extend)
    sync_call, first_out = GPS_SHAPE[extend]
    assert not np.any(g["flags"] & LOST) and g["state"][-1] == free["state"][-1]
    sync = np.nonzero(g["flags"] & gsdr.TRK_F_BIT_SYNC)[0]
    assert len(sync) == 1 and abs(int(sync[0]) - sync_call) <= 2
    assert (3 in g["state"]) == (extend > 1)
    s4 = g["state"] == 4
    assert abs(g["carrier_doppler_hz"][s4].mean() - tc.SAT.doppler_hz) <= 1.0
    _, _, dP, bar = _state_distances(x, P, g, lambda v: _gps_kf(conf, v)[0], "gps extend %d" % extend)
    assert 0 < bar and dP <= bar, (dP, bar)


@pytest.mark.parametrize("extend", [1, 4])
def test_gps_filter_state_x(extend):
    """x after the run against the replay's, within 100 times the distance between the two
    CPU evaluations.  That distance is below one place of x(1) (the two agree in x(1) and x(2)
    bit for bit), so the bar asks the same of the device: it is met because the device sums
    every product in the restatement's order and evaluates the float library calls that
    feed the filter correctly rounded, as the restatement does (kf_restatement.py).  With the
    device's own atanf / hypotf and another product order x was 1.5e-10 of max|x| away."""
    g, x, P, _ = _gps_gpu_run(extend)
    conf = _gps_conf(extend)
    dx, bar, _, _ = _state_distances(x, P, g, lambda v: _gps_kf(conf, v)[0], "gps extend %d" % extend)
    assert dx <= bar, (dx, bar)


@functools.lru_cache(maxsize=None)
def _gal_gpu_run():
    conf, iq, code, dcode, delay, dop, prn = _oracle_scenario("gal_pilot")
    t = gsdr.Tracking(conf)
    t.set_kf()
    first = t.start(0, prn, code, delay, dop, 0, 0, data_code=dcode)
    rec, n = t.run(iq, 0, 320)
    g = rec[0][:n[0]].copy()
    x, P = t.kf_state(0)
    t.close()
    g.setflags(write=False)
    return g, x, P, first


def _gal_make(first):
    conf, _, code, dcode, delay, dop, prn = _oracle_scenario("gal_pilot")

    def make(variant):
        ch = kr.KfChannel(conf[0:1].view(trk.TRK_CONF_DTYPE), variant=variant)
        assert ch.start(code, delay, dop, 0, 0, prn=prn, data_code=dcode) == first
        return ch
    return make


def test_gal_pilot_filter_state_x():
    """As test_gps_filter_state_x, on the four-quadrant discriminator after the hand-over."""
    g, x, P, first = _gal_gpu_run()
    dx, bar, _, _ = _state_distances(x, P, g, _gal_make(first), "gal_pilot")
    assert dx <= bar, (dx, bar)


def test_gal_pilot_loop_parity():
    conf, iq, code, dcode, delay, dop, prn = _oracle_scenario("gal_pilot")
    g, x, P, first = _gal_gpu_run()
    make = _gal_make(first)
    assert len(g) == 320
    c0 = conf[0]
    el, vel = float(c0["early_late_space_chips"]), float(c0["very_early_late_space_chips"])
    assert _open_loop_sig(g, iq, code, dcode, FS, dop, [-vel, -el, 0.0, el, vel], 2, 1.023e6, 8000, 2) <= 1e-4
    o = _replay_check(g, make("ref"), "kf gal_pilot")
    free, _, _ = gal_free_run()
    if not np.any(free["flags"] & LOST):
        assert not np.any(g["flags"] & LOST) and g["state"][-1] == free["state"][-1]
    print("gal_pilot: cn0_db_hz GPU vs replay, calls that differ %d, max %.3e dB" %
          (np.count_nonzero(g["cn0_db_hz"] != o["cn0_db_hz"]), np.max(np.abs(g["cn0_db_hz"] - o["cn0_db_hz"]))))


def test_gal_pilot_filter_covariance():
    """P after the run against the replay's, within 100 times the distance between the two CPU
    evaluations.  In state 4 R is rebuilt from the call's C/N0: with the float estimator's own
    log10f the device's C/N0 was a last place off numpy's in some calls and P 8.1e-11 of max|P|
    away; with the logarithm correctly rounded on both sides the C/N0 agrees in every call
    (test_gal_pilot_loop_parity prints it) and P meets the bar."""
    g, x, P, first = _gal_gpu_run()
    _, _, dP, bar = _state_distances(x, P, g, _gal_make(first), "gal_pilot")
    assert 0 < bar and dP <= bar, (dP, bar)


def test_channels_do_not_mix():
    sats = [tc.SAT, synth.Satellite(12, -2200.0, 77.7, 47.0, 1.1, code_doppler=True),
            synth.Satellite(20, 2990.0, 640.4, 46.0, 2.1, code_doppler=True)]
    iq = synth.gps_l1_iq(FS, int(0.3 * FS), sats, seed_offset=5)
    starts = [(s.prn,) + tc._acq(s, FS) for s in sats]
    calls = 280

    def run(chans):
        t = gsdr.Tracking(_gps_conf(1, len(chans)))
        t.set_kf()
        for i, (prn, delay, dop) in enumerate(chans):
            t.start(i, prn, synth.gps_ca_chips(prn), delay, dop, 0, tc.NITEMS)
        rec, n = t.run(iq, 0, calls)
        return [rec[i][:n[i]].copy() for i in range(len(chans))], [t.kf_state(i) for i in range(len(chans))]
    pool, pool_state = run(starts)
    for i, s in enumerate(starts):
        single, single_state = run([s])
        assert len(pool[i]) == calls
        assert pool[i].tobytes() == single[0].tobytes(), i
        np.testing.assert_array_equal(pool_state[i][0], single_state[0][0])
        np.testing.assert_array_equal(pool_state[i][1], single_state[0][1])
    assert not np.array_equal(pool_state[0][0], pool_state[1][0])


def test_save_and_restore_carry_the_filter():
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    t = gsdr.Tracking(_gps_conf())
    t.set_kf()
    t.start(0, prn, synth.gps_ca_chips(prn), delay, dop, 0, tc.NITEMS)
    t.run(iq, 0, 200)
    t.save_state(0)
    a, na = t.run(iq, 0, 100)
    xa, Pa = t.kf_state(0)
    t.restore_state(0)
    b, nb = t.run(iq, 0, 100)
    xb, Pb = t.kf_state(0)
    assert na[0] == nb[0] == 100
    assert a[0].tobytes() == b[0].tobytes()
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(Pa, Pb)
    assert xa[2] != dop and Pa[2, 2] != 25.0  # the filter did move


def test_forced_loss_and_restart():
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    code = synth.gps_ca_chips(prn)
    conf = _gps_conf()
    t = gsdr.Tracking(conf)
    t.set_kf()
    t.start(0, prn, code, delay, dop, 0, tc.NITEMS)
    head, n = t.run(iq, 0, 1200)
    head = head[0][:n[0]]
    assert n[0] == 1200 and head["state"][-1] == 4
    x0, P0 = t.kf_state(0)
    t.force_loss_of_lock(0)
    tail, n2 = t.run(iq, 0, 5)
    assert n2[0] == 1
    g = np.concatenate([head, tail[0][:1]])
    assert g["flags"][-1] & LOST and g["state"][-1] == 4 and t.channel(0)["state"] == 0
    rep, _ = _gps_kf(conf)
    o = rep.replay(g, force_before=(1200,))
    for f in ("sample_counter", "consumed", "state", "flags", "prompt_i", "prompt_q"):
        np.testing.assert_array_equal(g[f], o[f], err_msg=f)
    for f, tol in (("carrier_doppler_hz", 1e-2), ("code_freq_chips", 1e-4), ("rem_code_phase_samples", 1e-4),
                   ("cn0_db_hz", 1e-3), ("carrier_lock_test", 1e-4), ("carr_phase_error_hz", 1e-3),
                   ("carr_error_filt_hz", 1e-2), ("code_error_chips", 1e-4), ("code_error_filt_chips", 1e-3)):
        assert np.max(np.abs(g[f].astype(np.float64) - o[f])) <= tol, f
    # the lost call's filter step is dropped
    x1, P1 = t.kf_state(0)
    np.testing.assert_array_equal(x0, x1)
    np.testing.assert_array_equal(P0, P1)
    # a new start: init_kf
    t.start(0, prn, code, delay, 1500.0, 0, tc.NITEMS)
    x, P = t.kf_state(0)
    np.testing.assert_array_equal(x, [0.0, 0.0, 1500.0, 0.0])
    np.testing.assert_array_equal(P, np.diag([0.5 ** 2, 0.7 ** 2, 5.0 ** 2, 1.0 ** 2]))


def test_ring_path_matches_run():
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    code = synth.gps_ca_chips(prn)
    calls, vl = 64, 2000
    n_items = (calls + 4) * vl
    a = gsdr.Tracking(_gps_conf())
    a.set_kf()
    a.start(0, prn, code, delay, dop, 0, tc.NITEMS)
    want, nw = a.run(iq[:n_items], 0, calls)
    b = gsdr.Tracking(_gps_conf())
    b.set_kf()
    b.start(0, prn, code, delay, dop, 0, tc.NITEMS)
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=2 * n_items, max_window_items=n_items)
    ring.push(iq[:n_items], 0)
    got, ng = b.run_stream_host(ring, calls)
    assert nw[0] == ng[0] == calls
    assert want[0].tobytes() == got[0].tobytes()
    np.testing.assert_array_equal(a.kf_state(0)[1], b.kf_state(0)[1])


def _short_dll_pll_run(t):
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    t.start(0, prn, synth.gps_ca_chips(prn), delay, dop, 0, tc.NITEMS)
    rec, n = t.run(iq[:130 * 2000], 0, 120)
    assert n[0] == 120
    return rec[0].tobytes()


def test_refusals_leave_the_handle_as_it_was():
    fresh = _short_dll_pll_run(gsdr.Tracking(_gps_conf()))
    # a negative and a non-finite value
    for bad in (-0.1, float("nan"), float("inf")):
        t = gsdr.Tracking(_gps_conf())
        c = gsdr.trk_kf_conf_default()
        c["carrier_freq_sd_hz"] = bad
        with pytest.raises(gsdr.GsdrError) as e:
            t.set_kf(c)
        assert e.value.code == gsdr.GSDR_E_ARG
        with pytest.raises(gsdr.GsdrError) as e:
            t.kf_state(0)  # still a DLL/PLL handle
        assert e.value.code == gsdr.GSDR_E_STATE
        assert _short_dll_pll_run(t) == fresh
    # after a start
    t = gsdr.Tracking(_gps_conf())
    assert _short_dll_pll_run(t) == fresh
    with pytest.raises(gsdr.GsdrError) as e:
        t.set_kf()
    assert e.value.code == gsdr.GSDR_E_STATE
    t.stop(0)
    assert _short_dll_pll_run(t) == fresh
    # high dynamics
    hd = _gps_conf()
    hd["high_dyn"] = 1
    fresh_hd = _short_dll_pll_run(gsdr.Tracking(hd))
    t = gsdr.Tracking(hd)
    with pytest.raises(gsdr.GsdrError) as e:
        t.set_kf()
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED
    assert _short_dll_pll_run(t) == fresh_hd


# ------------------------------------------------------------------ Galileo E5a pilot (compact replicas)
def test_e5a_pilot_loop_parity():
    """The 10230-chip pilot case in Kalman mode: two float replicas do not fit a CU's LDS beside the
    input buffers, so the handle launches the compact-replica Kalman instance, as the
    DLL/PLL loop does; taps, loop and secondary-code synchronisation against the restatement."""
    import trk_wideband_checks as wb
    c = wb.case("5X", 1)
    t = gsdr.Tracking(c.conf(1))
    t.set_kf()
    first = t.start(0, c.prn, c.code, c.delay, c.dop, 0, 0, data_code=c.data_code, secondary_code=c.secondary)
    assert first == c.first
    rec, n = t.run(c.iq, 0, 260)
    g = rec[0][:n[0]]
    x, P = t.kf_state(0)
    t.close()
    assert len(g) == 260
    assert _open_loop_sig(g, c.iq, c.code, c.data_code, c.fs, c.dop, [-0.25, 0.0, 0.25], 1, wb.CHIP_RATE, c.vl, 1) <= 1e-4

    def make(variant):
        ch = kr.KfChannel(c.conf()[0:1].view(trk.TRK_CONF_DTYPE), secondary_code=c.secondary, variant=variant)
        assert ch.start(c.code, c.delay, c.dop, 0, 0, prn=c.prn, data_code=c.data_code) == first
        return ch
    _replay_check(g, make("ref"), "kf e5a pilot")
    dx, bx, dP, bP = _state_distances(x, P, g, make, "e5a pilot")
    assert dx <= bx and dP <= bP, (dx, bx, dP, bP)


# ------------------------------------------------------------------ host adapter
import json
import os
import subprocess

KF_EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnss-sdr-new_amd", "build",
                      "kf_tracking_selftest")


def _kf_selftest(tmp_path, iq, prn, delay, dop, pooled, extra=()):
    (tmp_path / "iq.dat").write_bytes(np.ascontiguousarray(iq, np.complex64).tobytes())
    lines = ["GNSS-SDR.internal_fs_sps=%d" % int(FS), "Tracking_1C.implementation=GPS_L1_CA_KF_Tracking_MI355X",
             "Tracking_1C.item_type=gr_complex", "Tracking_1C.pull_in_time_s=0", "Channels_1C.count=1",
             "Tracking_1C.mi355x_pool=%s" % ("true" if pooled else "false")] + list(extra)
    (tmp_path / "trk.conf").write_text("\n".join(lines) + "\n")
    p = subprocess.run([KF_EXE, str(tmp_path / "trk.conf"), str(tmp_path / "iq.dat"), "Tracking_1C", str(prn), repr(delay),
                        repr(dop)], capture_output=True, text=True, timeout=120)
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("pooled", [False, True])
def test_host_adapter_emits_the_c_abi_records(tmp_path, pooled):
    """GPS_L1_CA_KF_Tracking_MI355X built by the block factory from a .conf: the Gnss_Synchro sequence of
    the block (per channel and pooled) equals the valid outputs of the C ABI driven directly with Kf_Conf's
    values, and the adapter applies the reference's rules to the configuration."""
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    rc, r = _kf_selftest(tmp_path, iq, prn, delay, dop, pooled,
                         ["Tracking_1C.extend_correlation_symbols=25", "Tracking_1C.track_pilot=true",
                          "Tracking_1C.carrier_freq_sd_hz=0.5"])
    assert rc == 0 and r["built"] and r["pooled"] == pooled and r["vector_length"] == 2000, r.get("error")
    assert r["kf"] and r["extend"] == 20 and not r["track_pilot"] and r["bit_sync_limit_s"] == 60
    c = gsdr.trk_conf_default()  # what Kf_Conf makes of that .conf
    c["fs_in"], c["pull_in_time_s"], c["bit_synchronization_time_limit_s"], c["extend_correlation_symbols"] = FS, 0, 60, 20
    kc = gsdr.trk_kf_conf_default()
    kc["carrier_freq_sd_hz"] = 0.5
    t = gsdr.Tracking(c)
    t.set_kf(kc)
    t.start(0, prn, synth.gps_ca_chips(prn), delay, dop, 0, 0)
    rec, n = t.run(iq, 0, GPS_CALLS)
    g = rec[0][:n[0]]
    v = g[(g["flags"] & gsdr.TRK_F_VALID_OUTPUT) != 0]
    outs = r["outputs"]
    m = min(len(outs), len(v))
    assert len(v) - 1 <= len(outs) <= len(v) + 1 and m >= 5, (len(outs), len(v))
    for o, e in zip(outs[:m], v[:m]):
        assert o[0] == int(e["sample_counter"]) and o[1] == e["prompt_i"] and o[2] == e["prompt_q"], (o, e)
        assert o[3] == 1 and o[4] == 1
    for o, e in zip(outs[:m], r["records"][:m]):
        assert o[:3] == e[:3]


def test_host_adapter_refuses_high_dynamics(tmp_path):
    iq, _, (prn, delay, dop) = tc.scenario_input("signal")
    rc, r = _kf_selftest(tmp_path, iq[:20000], prn, delay, dop, False, ["Tracking_1C.high_dyn=true"])
    assert rc == 1 and not r["built"] and "high-dynamics" in r["error"]

"""GPU parity of the device-resident DLL/PLL tracking loop (gsdr_trk_*) against the
CPU restatement of dll_pll_veml_tracking (oracle/trk_oracle.c) on the same
synthetic IQ.  Three checks per channel:

1. correlation, open loop (north_star 1e-4 relative fp32): every call's E/P/L taps
   against the oracle correlator (generic VOLK resampler + rotator) fed with the
   NCO state the GPU carried into that call (recovered from the previous record):
   vector-norm relative <= 1e-4 for every call.
2. loop, replay: the oracle channel driven call by call with the GPU's own taps
   (orc_trk_call_taps) must reproduce the GPU's loop: identical schedule (sample
   counter, consumed, state, flags), Prompt_I/Q bit-identical, Doppler / code rate /
   code and carrier remainders / CN0 / lock test to device-math rounding.
3. loop, free running (sanity): the two loops run independently on the same input
   agree on the schedule and outputs except where a rounding-level state difference
   moves one sample across a chip or sample boundary now and then -- the
   reference's float code index is that sensitive, which is why 1
   and 2 pin the kernel and the loop separately.
"""
import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import trk

from trk_checks import (_acq, _conf, _conf_sig, _free_check, _open_loop_hd, _open_loop_sig,  # noqa: F401
                        _open_loop_taps, _oracle_channel, _oracle_sig, _replay_check)

pytestmark = pytest.mark.gpu


def test_single_channel_matches_oracle_through_bit_sync():
    fs = 2.0e6
    sat = synth.Satellite(7, 1234.5, 300.3, 45.0, 0.7, preamble_every_bits=25, code_doppler=True)
    iq = synth.gps_l1_iq(fs, int(2.2 * fs), [sat], seed_offset=5)
    delay, dop = _acq(sat, fs)
    code = synth.gps_ca_chips(7)
    t = gsdr.Tracking(_conf(fs))
    first_g = t.start(0, 7, code, delay, dop, 0, 2000)
    rec, n = t.run(iq, 0, 3000)
    g = rec[0][:n[0]]
    free, first_o = _oracle_channel(fs, code, delay, dop, 2000)
    assert first_g == first_o
    assert _open_loop_taps(g, iq, code, fs, dop) <= 1e-4
    _replay_check(g, _oracle_channel(fs, code, delay, dop, 2000)[0], "single")
    orc, _ = free.run(iq, 0, first_o, 3000)
    _free_check(g, orc, "single")
    assert g["state"][-1] == 4 and np.any(g["flags"] & gsdr.TRK_F_BIT_SYNC)
    assert np.count_nonzero(g["flags"] & gsdr.TRK_F_VALID_OUTPUT) > 10


@pytest.mark.parametrize("item", [gsdr.ITEM_GR_COMPLEX, gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_channel_pool_across_launches(item):
    """8 channels in one launch per chunk; the loop state persists on the device
    between launches (chunked input, like consecutive GNU Radio buffers)."""
    fs = 2.0e6
    sats = synth.random_constellation(8, seed_offset=41, cn0_dbhz=46.0)
    for s in sats:
        s.preamble_every_bits = 25
        s.code_doppler = True
    iq = synth.gps_l1_iq(fs, int(1.8 * fs), sats, seed_offset=41)
    if item == gsdr.ITEM_CSHORT:
        host = synth.to_cshort(iq, 800.0)
        iq_ref = (host[0::2].astype(np.float32) + 1j * host[1::2].astype(np.float32)).astype(np.complex64)
    elif item == gsdr.ITEM_IBYTE:
        host = synth.to_ibyte(iq, 16.0)
        iq_ref = synth.ibyte_to_complex(host)
    else:
        host = iq
        iq_ref = iq
    t = gsdr.Tracking(_conf(fs, 8, item))
    starts = []
    for c, s in enumerate(sats):
        delay, dop = _acq(s, fs)
        fg = t.start(c, s.prn, synth.gps_ca_chips(s.prn), delay, dop, 0, 2000)
        starts.append((delay, dop, fg))
    # four launches over overlapping windows of the stream
    got = [[] for _ in sats]
    n_total = len(iq_ref)
    bounds = [0, n_total // 4, n_total // 2, (3 * n_total) // 4, n_total]
    for k in range(4):
        lo = max(0, bounds[k] - 8000)
        hi = bounds[k + 1]
        chunk = host[2 * lo:2 * hi] if item != gsdr.ITEM_GR_COMPLEX else host[lo:hi]
        rec, n = t.run(chunk, lo, 2000)
        for c in range(len(sats)):
            got[c].append(rec[c][:n[c]])
    for c, s in enumerate(sats):
        delay, dop, fg = starts[c]
        code = synth.gps_ca_chips(s.prn)
        g = np.concatenate(got[c])
        assert np.all(np.diff(g["sample_counter"].astype(np.int64)) == g["consumed"][:-1]), c
        assert _open_loop_taps(g, iq_ref, code, fs, dop) <= 1e-4
        _replay_check(g, _oracle_channel(fs, code, delay, dop, 2000)[0], "ch%d" % c)
        free, fo = _oracle_channel(fs, code, delay, dop, 2000)
        assert fo == fg
        orc, _ = free.run(iq_ref, 0, fo, 4000)
        _free_check(g, orc, "ch%d" % c)


@pytest.mark.parametrize("at", [300, 2000])
def test_telemetry_fault_forces_loss_of_lock(at):
    """msg_handler_telemetry_to_trk (dll_pll_veml_tracking.cc:614-637): a telemetry
    fault between two calls sets the carrier lock fail counter to 200000, so the next
    call's lock check (state 2 in the pull-in transitory at call 300, state 4 after
    bit sync at call 2000) reports the loss of lock: the GPU's records, replayed
    through the oracle with the fault before the same call, agree flag for flag."""
    fs = 2.0e6
    sat = synth.Satellite(7, 1234.5, 300.3, 45.0, 0.7, preamble_every_bits=25, code_doppler=True)
    iq = synth.gps_l1_iq(fs, int(2.4 * fs), [sat], seed_offset=5)
    delay, dop = _acq(sat, fs)
    code = synth.gps_ca_chips(7)
    t = gsdr.Tracking(_conf(fs))
    t.start(0, 7, code, delay, dop, 0, 2000)
    a, na = t.run(iq, 0, at)
    assert na[0] == at
    t.force_loss_of_lock(0)
    b, nb = t.run(iq, 0, 3000)
    g = np.concatenate([a[0][:na[0]], b[0][:nb[0]]])
    # the fault's call is the last one: loss of lock, channel back to standby
    assert len(g) == at + 1, len(g)
    assert g["flags"][at] & gsdr.TRK_F_LOSS_OF_LOCK and not np.any(g["flags"][:at] & gsdr.TRK_F_LOSS_OF_LOCK)
    assert g["state"][at] == (2 if at < 1000 else 4)
    assert t.channel(0)["state"] == 0
    o = _oracle_channel(fs, code, delay, dop, 2000)[0].replay(g, force_before=[at])
    for f in ("sample_counter", "consumed", "state", "flags"):
        np.testing.assert_array_equal(g[f], o[f], err_msg=f)
    np.testing.assert_array_equal(g["prompt_i"], o["prompt_i"])
    # without the fault the oracle keeps the lock through the same calls
    o2 = _oracle_channel(fs, code, delay, dop, 2000)[0].replay(g)
    assert not np.any(o2["flags"] & gsdr.TRK_F_LOSS_OF_LOCK)


def test_save_restore_replays_identically():
    fs = 2.0e6
    sat = synth.Satellite(12, -2200.0, 77.7, 47.0, 1.1, code_doppler=True)
    iq = synth.gps_l1_iq(fs, int(0.3 * fs), [sat], seed_offset=6)
    delay, dop = _acq(sat, fs)
    t = gsdr.Tracking(_conf(fs))
    t.start(0, 12, synth.gps_ca_chips(12), delay, dop, 0, 2000)
    t.save_state(0)
    a, na = t.run(iq, 0, 100)
    st = t.channel(0)
    t.restore_state(0)
    b, nb = t.run(iq, 0, 100)
    assert na[0] == nb[0] == 100
    assert a.tobytes() == b.tobytes()
    assert t.channel(0) == st


def test_stop_and_standby_consume_nothing():
    fs = 2.0e6
    sat = synth.Satellite(3, 500.0, 10.0, 45.0)
    iq = synth.gps_l1_iq(fs, int(0.05 * fs), [sat], seed_offset=7)
    t = gsdr.Tracking(_conf(fs, 2))
    t.start(1, 3, synth.gps_ca_chips(3), 20.0, 500.0, 0, 0)
    t.stop(1)
    rec, n = t.run(iq, 0, 50)
    assert list(n) == [0, 0]
    assert t.channel(1)["state"] == 0


# ---------------------------------------------------------------- Galileo E1 / BeiDou B1I
@pytest.mark.parametrize("pilot", [1, 0])
def test_galileo_e1_matches_oracle(pilot):
    """Config C4's signal: Galileo E1 VEML 5 taps (+ the E1B data prompt when
    tracking the E1C pilot), 4 ms calls, E1C secondary-code lock."""
    fs = 4.0e6
    sat = synth.GalileoSatellite(11, 1234.5, 1000.3, 50.0, 0.7)
    iq = synth.gal_e1_iq(fs, int(1.5 * fs), [sat], seed_offset=5)
    tau = sat.code_delay_chips / (1.023e6 * (1 + sat.doppler_hz / 1.57542e9)) * fs
    delay, dop = float(round(tau) % 16000), 1250.0
    code = synth.gal_e1_sinboc11(11, pilot=bool(pilot))
    dcode = synth.gal_e1_sinboc11(11) if pilot else None
    t = gsdr.Tracking(_conf_sig(fs, gsdr.SIGNAL_GAL_1B, 1, pilot))
    fg = t.start(0, 11, code, delay, dop, 0, 0, data_code=dcode)
    rec, n = t.run(iq, 0, 400)
    g = rec[0][:n[0]]
    free, fo = _oracle_sig(fs, 1, pilot, code, dcode, delay, dop, 0, 11)
    assert fg == fo
    el, vel = 0.25, 0.5
    assert _open_loop_sig(g, iq, code, dcode, fs, dop, [-vel, -el, 0.0, el, vel], 2, 1.023e6, 16000, 2) <= 1e-4
    _replay_check(g, _oracle_sig(fs, 1, pilot, code, dcode, delay, dop, 0, 11)[0], "gal%d" % pilot)
    orc, _ = free.run(iq, 0, fo, 400)
    _free_check(g, orc, "gal%d" % pilot)
    assert g["state"][-1] == 4 and np.count_nonzero(g["flags"] & gsdr.TRK_F_BIT_SYNC) == 1


@pytest.mark.parametrize("prn", [14, 3])
def test_beidou_b1i_matches_oracle(prn):
    """Config C5's BeiDou signal: B1I D1 (NH code lock, NH wiped from the 20 ms
    symbols) and D2 GEO (preamble search, 2 ms symbols)."""
    fs = 4.0e6
    s = synth.Satellite(prn, -2262.3, 500.2, 45.0, 0.3)
    iq = synth.bds_b1i_iq(fs, int(1.5 * fs), [s], seed_offset=7)
    tau = s.code_delay_chips / (2.046e6 * (1 + s.doppler_hz / 1.561098e9)) * fs
    delay, dop = float(round(tau) % 4000), -2250.0
    code = synth.bds_b1i_chips(prn)
    t = gsdr.Tracking(_conf_sig(fs, gsdr.SIGNAL_BDS_B1))
    fg = t.start(0, prn, code, delay, dop, 0, 0)
    rec, n = t.run(iq, 0, 1480)
    g = rec[0][:n[0]]
    free, fo = _oracle_sig(fs, 2, 0, code, None, delay, dop, 0, prn)
    assert fg == fo
    assert _open_loop_sig(g, iq, code, None, fs, dop, [-0.25, 0.0, 0.25], 1, 2.046e6, 4000, 1) <= 1e-4
    _replay_check(g, _oracle_sig(fs, 2, 0, code, None, delay, dop, 0, prn)[0], "bds%d" % prn)
    orc, _ = free.run(iq, 0, fo, 1480)
    _free_check(g, orc, "bds%d" % prn)
    assert g["state"][-1] == 4
    out = np.nonzero(g["flags"] & gsdr.TRK_F_VALID_OUTPUT)[0]
    assert len(out) > 5 and np.all(np.diff(out) == (2 if synth.bds_is_geo(prn) else 20))


@pytest.mark.parametrize("sig", ["gal_c4", "gps_ext10"])
def test_extended_integration_matches_oracle(sig):
    """Extended coherent integration (state 3, dll_pll_veml_tracking.cc:1945-2026):
    config C4's Galileo E1 settings (conf/gnss-sdr_galileo_E1_extended_correlator_byte.conf:
    4 symbols, narrow PLL/DLL, narrow VEML taps) and GPS L1 C/A over 10 ms."""
    if sig == "gal_c4":
        fs = 4.0e6
        sat = synth.GalileoSatellite(11, 1234.5, 1000.3, 50.0, 0.7)
        iq = synth.gal_e1_iq(fs, int(1.6 * fs), [sat], seed_offset=5)
        tau = sat.code_delay_chips / (1.023e6 * (1 + sat.doppler_hz / 1.57542e9)) * fs
        delay, dop, prn = float(round(tau) % 16000), 1250.0, 11
        code, dcode = synth.gal_e1_sinboc11(11, pilot=True), synth.gal_e1_sinboc11(11)
        c = _conf_sig(fs, gsdr.SIGNAL_GAL_1B, 1, 1)
        c["pll_bw_hz"], c["dll_bw_hz"] = 15.0, 1.0
        c["pll_bw_narrow_hz"], c["dll_bw_narrow_hz"] = 5.0, 0.25
        c["early_late_space_chips"], c["very_early_late_space_chips"] = 0.15, 0.6
        c["early_late_space_narrow_chips"], c["very_early_late_space_narrow_chips"] = 0.06, 0.25
        c["extend_correlation_symbols"] = 4
        wide, narrow, spc, rate, vl, iP, n_calls, osig = [-0.6, -0.15, 0, 0.15, 0.6], [-0.25, -0.06, 0, 0.06, 0.25], 2, \
            1.023e6, 16000, 2, 380, 1
    else:
        fs = 2.0e6
        sat = synth.Satellite(7, 1234.5, 300.3, 45.0, 0.7, preamble_every_bits=25, code_doppler=True)
        iq = synth.gps_l1_iq(fs, int(2.0 * fs), [sat], seed_offset=5)
        delay, dop = _acq(sat, fs)
        prn, code, dcode = 7, synth.gps_ca_chips(7), None
        c = _conf(fs)
        c["extend_correlation_symbols"] = 10
        wide, narrow, spc, rate, vl, iP, n_calls, osig = [-0.25, 0, 0.25], [-0.15, 0, 0.15], 1, 1.023e6, 2000, 1, 1990, 0
    t = gsdr.Tracking(c)
    fg = t.start(0, prn, code, delay, dop, 0, 0, data_code=dcode)
    rec, n = t.run(iq, 0, n_calls)
    g = rec[0][:n[0]]
    oc = c[0:1].view(trk.TRK_CONF_DTYPE)
    free = trk.Channel(oc)
    fo = free.start(code, delay, dop, 0, 0, prn=prn, data_code=dcode)
    assert fg == fo
    assert _open_loop_sig(g, iq, code, dcode, fs, dop, wide, spc, rate, vl, iP, narrow) <= 1e-4
    rep = trk.Channel(oc)
    rep.start(code, delay, dop, 0, 0, prn=prn, data_code=dcode)
    _replay_check(g, rep, sig)
    orc, _ = free.run(iq, 0, fo, n_calls)
    _free_check(g, orc, sig)
    st = set(np.unique(g["state"]).tolist())
    assert {2, 3, 4} <= st


@pytest.mark.parametrize("smoother", [10, 3])
def test_high_dynamics_loop_matches_oracle(smoother):
    """high_dyn = true (dll_pll_veml_tracking.cc:527-533, :1232-1284): carrier and code
    rate estimates from the step histories drive the high-dynamics resampler/rotator.
    A 60 Hz/s Doppler ramp; replay (the oracle loop on the GPU's taps: histories and
    rates bit-identical) and free-running agreement with the oracle's generic VOLK
    high-dynamics kernels."""
    fs = 2.0e6
    sat = synth.Satellite(9, -1500.0, 512.2, 46.0, 0.3, preamble_every_bits=25, code_doppler=True,
                          doppler_rate_hz_s=60.0)
    iq = synth.gps_l1_iq(fs, int(1.6 * fs), [sat], seed_offset=8)
    delay, dop = _acq(sat, fs)
    code = synth.gps_ca_chips(9)
    conf = _conf(fs)
    conf["high_dyn"] = 1
    conf["smoother_length"] = smoother
    t = gsdr.Tracking(conf)
    first_g = t.start(0, 9, code, delay, dop, 0, 2000)
    rec, n = t.run(iq, 0, 2000)
    g = rec[0][:n[0]]
    free, first_o = _oracle_channel(fs, code, delay, dop, 2000, conf)
    assert first_g == first_o
    # open loop: every call's taps against the oracle's high-dynamics resampler and
    # rotator, fed the rate steps of the previous record.  Those floats are the
    # correlator's input on both sides (the kernel rounds its double rates to float
    # in Prep as do_correlation_step's casts do), so the bound needs no allowance.
    assert _open_loop_hd(g, iq, code, fs, dop) <= 1e-4
    _replay_check(g, _oracle_channel(fs, code, delay, dop, 2000, conf)[0], "hd%d" % smoother)
    orc, _ = free.run(iq, 0, first_o, 2000)
    _free_check(g, orc, "hd%d" % smoother)
    # the loop follows the ramp: final Doppler near -1500 + 60 * t
    t_end = float(g["sample_counter"][-1]) / fs
    assert abs(float(g["carrier_doppler_hz"][-1]) - (-1500.0 + 60.0 * t_end)) < 10.0
    assert g["state"][-1] == 4
    # the rate estimates are live once the histories are full (2 * smoother_length calls)
    assert np.all(g["carrier_rate"][:2 * smoother - 1] == 0.0)
    assert np.count_nonzero(g["carrier_rate"]) > len(g) // 2 and np.count_nonzero(g["code_rate"]) > len(g) // 2
    # mean carrier rate ~ the ramp: 2*pi*60/fs^2 rad/sample^2 (noisy per call)
    want = 2 * np.pi * 60.0 / fs ** 2
    assert abs(np.mean(g["carrier_rate"][len(g) // 2:]) - want) < 0.5 * want


def test_high_dynamics_conf_limits():
    conf = _conf(2.0e6)
    conf["high_dyn"] = 1
    conf["smoother_length"] = 33
    with pytest.raises(gsdr.GsdrError):
        gsdr.Tracking(conf)

"""Oracle comparisons and scenarios shared by the tracking tests (not a test module).

The three checks of test_gpu_trk.py (its docstring states them): open-loop taps
against the oracle correlator, the oracle loop replayed on the GPU's taps, and the
free-running comparison.  Below them the scenario table of the loop options and the
lock losses, read by test_gpu_trk_loop_options.py (GPU against oracle) and by
test_oracle_tracking.py (the oracle alone, no GPU).
"""
import functools

import numpy as np

import gsdr
from gsdr import synth
from oracle import trk, volk

from conftest import ccompare, vnorm_rel

TWO_PI = 2.0 * 3.1415926535898  # MATH_CONSTANTS.h:47-49


def _conf(fs, nch=1, item=gsdr.ITEM_GR_COMPLEX):
    c = gsdr.trk_conf_default()
    c["fs_in"] = fs
    c["pll_bw_hz"] = 40.0  # conf/gnss-sdr_GPS_L1_gr_complex.conf:66-67
    c["dll_bw_hz"] = 4.0
    c["pull_in_time_s"] = 0
    c["max_channels"] = nch
    c["item_type"] = item
    return c


def _conf_sig(fs, sig, nch=1, pilot=1):
    c = _conf(fs, nch)
    c["signal"] = sig
    c["track_pilot"] = pilot
    c["pll_bw_hz"] = 15.0
    c["dll_bw_hz"] = 1.0
    return c


def _acq(sat, fs):
    """What an acquisition at stamp 0 would report: code start sample and grid Doppler."""
    tau = sat.code_delay_chips / (1.023e6 * (1 + sat.doppler_hz / 1.57542e9)) * fs
    return float(round(tau) % round(fs / 1000)), float(250 * round(sat.doppler_hz / 250))


def _in_noise(n0, vl, noise_spans):
    """True when the call's samples [n0, n0 + vl) lie wholly inside a noise-only span."""
    return any(lo <= n0 and n0 + vl <= hi for lo, hi in noise_spans)


def _open_loop_taps(g, iq, code, fs, acq_dop, el=0.25, noise_spans=()):
    """Oracle correlation of every GPU call with the GPU's own incoming NCO state.
    noise_spans: [lo, hi) sample ranges of iq that hold no signal.  A tap of a call
    inside one is a sum of noise that can land anywhere near zero, where the per-tap
    metric divides by it; those calls are held to the same 1e-4 as a vector norm over
    the call's taps (vnorm_rel).  Every other call is compared per tap as before."""
    shifts = np.array([-el, 0.0, el], np.float32)
    vl = int(round(fs / 1000))
    worst = 0.0
    for e in range(len(g)):
        if e == 0:
            rem_carr, dop, rem_samples, code_freq = 0.0, acq_dop, 0.0, 1.023e6
        else:
            p = g[e - 1]
            rem_carr, dop = float(p["rem_carr_phase_rad"]), float(p["carrier_doppler_hz"])
            rem_samples, code_freq = float(p["rem_code_phase_samples"]), float(p["code_freq_chips"])
        carr_step = float(np.float32(TWO_PI * dop / fs))
        rem_code = float(np.float32(code_freq * rem_samples / fs))
        code_step = float(np.float32(code_freq / fs))
        n0 = int(g[e]["sample_counter"])
        x = iq[n0:n0 + vl]
        metric = vnorm_rel if _in_noise(n0, vl, noise_spans) else ccompare
        # per tap (ccompare, VOLK QA metric) against the rotator the reference runs on
        # x86 (u_avx / a_avx) and against the fp64 evaluation of the same model
        ref = volk.multicorrelator_real_codes_avx(x, code, shifts, rem_carr, carr_step, rem_code, code_step, vl)
        got = g["taps"][e][:6].view(np.complex64)
        exact = volk.multicorrelator_real_codes_exact(x, code, shifts, rem_carr, carr_step, rem_code, code_step, vl)
        assert metric(got, exact) <= 1e-4, (e, metric(got, exact))
        worst = max(worst, metric(got, ref))
    return worst


def _open_loop_hd(g, iq, code, fs, acq_dop, el=0.25):
    """_open_loop_taps for high_dyn = true: the oracle's generic high-dynamics
    resampler and rotator, fed the incoming NCO state and the rate steps of the
    previous record -- the floats do_correlation_step hands the correlator
    (dll_pll_veml_tracking.cc:1064-1089; the code rate times samples per chip, 1
    for GPS L1 C/A).  Returns the worst per-tap distance to that kernel."""
    shifts = np.array([-el, 0.0, el], np.float32)
    vl = int(round(fs / 1000))
    worst = 0.0
    for e in range(len(g)):
        if e == 0:
            rem_carr, dop, rem_samples, code_freq, carr_rate, code_rate = 0.0, acq_dop, 0.0, 1.023e6, 0.0, 0.0
        else:
            p = g[e - 1]
            rem_carr, dop = float(p["rem_carr_phase_rad"]), float(p["carrier_doppler_hz"])
            rem_samples, code_freq = float(p["rem_code_phase_samples"]), float(p["code_freq_chips"])
            carr_rate, code_rate = float(p["carrier_rate"]), float(p["code_rate"])
        carr_step = float(np.float32(TWO_PI * dop / fs))
        rem_code = float(np.float32(code_freq * rem_samples / fs))
        code_step = float(np.float32(code_freq / fs))
        n0 = int(g[e]["sample_counter"])
        x = iq[n0:n0 + vl]
        ref = volk.multicorrelator_real_codes(x, code, shifts, rem_carr, carr_step, rem_code, code_step, vl,
                                              carr_rate=carr_rate, code_rate=code_rate, high_dyn=True)
        got = g["taps"][e][:6].view(np.complex64)
        worst = max(worst, ccompare(got, ref))
    return worst


def _replay_check(g, oracle_channel, tag, bounds=None):
    """Check 2: the oracle loop fed with the GPU's taps reproduces the GPU's loop.
    bounds: measured bounds that replace the listed ones for single fields (only
    DLL3_BOUNDS and HD_RESTART_BOUNDS below); returns the oracle's records."""
    bounds = bounds or {}
    o = oracle_channel.replay(g)
    assert len(o) == len(g), (tag, len(o), len(g))
    for f in ("sample_counter", "consumed", "state", "flags"):
        np.testing.assert_array_equal(g[f], o[f], err_msg="%s %s" % (tag, f))
    np.testing.assert_array_equal(g["prompt_i"], o["prompt_i"], err_msg=tag)
    np.testing.assert_array_equal(g["prompt_q"], o["prompt_q"], err_msg=tag)
    for f in ("carrier_rate", "code_rate"):
        if f in bounds:
            d = np.max(np.abs(g[f].astype(np.float64) - o[f]))
            assert d <= bounds[f], (tag, f, d)
        else:
            np.testing.assert_array_equal(g[f], o[f], err_msg=tag)
    for f, tol in (("carrier_doppler_hz", 1e-2), ("code_freq_chips", 1e-4), ("rem_code_phase_samples", 1e-4),
                   ("acc_carrier_phase_rad", 1e-2), ("cn0_db_hz", 1e-3), ("carrier_lock_test", 1e-4),
                   ("evm", 1e-4)):
        d = np.max(np.abs(g[f] - o[f]))
        assert d <= bounds.get(f, tol), (tag, f, d)
    dr = np.abs(np.angle(np.exp(1j * (g["rem_carr_phase_rad"].astype(np.float64) - o["rem_carr_phase_rad"]))))
    assert dr.max() <= 5e-2, (tag, dr.max())  # integrates the float Doppler drift above
    # log_data's fields (the tracking dump): accumulator magnitudes and loop errors
    np.testing.assert_allclose(g["log_accu"], o["log_accu"], rtol=1e-5, atol=1e-3, err_msg=tag)
    for f, tol in (("carr_phase_error_hz", 1e-3), ("carr_error_filt_hz", 1e-2), ("code_error_chips", 1e-4),
                   ("code_error_filt_chips", 1e-3)):
        d = np.max(np.abs(g[f].astype(np.float64) - o[f]))
        assert d <= tol, (tag, f, d)
    return o


def _free_check(g, o, tag):
    """Check 3: independent loops agree up to rare boundary effects."""
    assert abs(len(g) - len(o)) <= 1, (tag, len(g), len(o))
    n = min(len(g), len(o))
    g, o = g[:n], o[:n]
    dsc = np.abs(g["sample_counter"].astype(np.int64) - o["sample_counter"].astype(np.int64))
    assert dsc.max() <= 1 and np.mean(dsc == 0) >= 0.95, (tag, dsc.max(), np.mean(dsc == 0))
    assert g["state"][-1] == o["state"][-1], tag
    sg = np.nonzero(g["flags"] & gsdr.TRK_F_BIT_SYNC)[0]
    so = np.nonzero(o["flags"] & gsdr.TRK_F_BIT_SYNC)[0]
    assert len(sg) == len(so) and np.all(np.abs(sg - so) <= 2), (tag, sg, so)
    dd = np.abs(g["carrier_doppler_hz"] - o["carrier_doppler_hz"])
    assert np.median(dd) <= 0.05 and dd.max() <= 5.0, (tag, np.percentile(dd, [50, 95, 100]))
    dc = np.abs(g["cn0_db_hz"] - o["cn0_db_hz"])
    assert np.median(dc) <= 0.02 and dc.max() <= 1.0, (tag, np.percentile(dc, [50, 95, 100]))


def _oracle_channel(fs, code, delay, dop, nitems, conf=None):
    ch = trk.Channel((_conf(fs) if conf is None else conf)[0:1].view(trk.TRK_CONF_DTYPE))
    first = ch.start(code, delay, dop, 0, nitems)
    return ch, first


def _open_loop_sig(g, iq, code, data_code, fs, acq_dop, shifts_chips, spc, chip_rate, vl, iP, narrow_chips=None,
                   spread=None, noise_spans=()):
    """Check 1 for any signal: every call's taps (and the data prompt) against the
    oracle correlator fed with the GPU's own incoming NCO state (narrow tap shifts
    in states 3/4 of the extended correlator), per tap (ccompare, the VOLK QA
    metric).  The bar: every tap within 1e-4 of the fp64 evaluation of
    the reference's correlation model and within 1e-4 of the rotator the reference
    dispatches on x86 (u_avx / a_avx, returned as the worst distance); the generic
    kernel's own fp32 phase drift reaches ~1e-4 at 100000 samples,
    so against it the GPU is held to 1e-4 beyond that kernel's own distance to fp64.
    spread (a dict) receives the worst per-tap distances over the calls.
    noise_spans: as in _open_loop_taps -- calls wholly inside a signal-free span of
    iq are measured by vnorm_rel over the call's taps, with the same bounds."""
    wide = (np.asarray(shifts_chips, np.float32) * np.float32(spc)).astype(np.float32)
    narrow = None if narrow_chips is None else (np.asarray(narrow_chips, np.float32) * np.float32(spc)).astype(np.float32)
    worst = 0.0
    for e in range(len(g)):
        shifts = narrow if (narrow is not None and g["state"][e] in (3, 4)) else wide
        if e == 0:
            rem_carr, dop, rem_samples, code_freq = 0.0, acq_dop, 0.0, chip_rate
        else:
            p = g[e - 1]
            rem_carr, dop = float(p["rem_carr_phase_rad"]), float(p["carrier_doppler_hz"])
            rem_samples, code_freq = float(p["rem_code_phase_samples"]), float(p["code_freq_chips"])
        carr_step = float(np.float32(TWO_PI * dop / fs))
        rem_code = float(np.float32(np.float32(code_freq * rem_samples / fs) * np.float32(spc)))
        code_step = float(np.float32(np.float32(code_freq / fs) * np.float32(spc)))
        n0 = int(g[e]["sample_counter"])
        x = iq[n0:n0 + vl]
        metric = vnorm_rel if _in_noise(n0, vl, noise_spans) else ccompare
        gen = volk.multicorrelator_real_codes(x, code, shifts, rem_carr, carr_step, rem_code, code_step, vl)
        avx = volk.multicorrelator_real_codes_avx(x, code, shifts, rem_carr, carr_step, rem_code, code_step, vl)
        exact = volk.multicorrelator_real_codes_exact(x, code, shifts, rem_carr, carr_step, rem_code, code_step, vl)
        got = g["taps"][e][:2 * len(shifts)].view(np.complex64)
        d = {"gpu_vs_fp64": metric(got, exact), "gpu_vs_avx": metric(got, avx), "gpu_vs_generic": metric(got, gen),
             "avx_vs_fp64": metric(avx, exact), "generic_vs_fp64": metric(gen, exact),
             "generic_vs_avx": metric(gen, avx)}
        assert d["gpu_vs_fp64"] <= 1e-4, (e, d)
        assert d["gpu_vs_generic"] <= 1e-4 + d["generic_vs_fp64"], (e, d)
        if spread is not None:
            for k, v in d.items():
                spread[k] = max(spread.get(k, 0.0), v)
            spread["calls"] = spread.get("calls", 0) + 1
        worst = max(worst, d["gpu_vs_avx"])
        if data_code is not None:
            refd = volk.multicorrelator_real_codes_avx(x, data_code, shifts[iP:iP + 1], rem_carr, carr_step, rem_code,
                                                       code_step, vl)
            worst = max(worst, ccompare(g["data_prompt"][e].view(np.complex64), refd))
    return worst


def _oracle_sig(fs, sig, pilot, code, data_code, delay, dop, nitems, prn):
    ch = trk.Channel(_conf_sig(fs, sig, 1, pilot)[0:1].view(trk.TRK_CONF_DTYPE))
    first = ch.start(code, delay, dop, 0, nitems, prn=prn, data_code=data_code)
    return ch, first


# ------------------------------------------------ loop options and lock losses: the scenarios
# GPS L1 C/A at 2 MHz, one channel, started as an acquisition at stamp 0 would with
# nitems_read = 2000, base configuration _conf(fs) (PLL 40 Hz, DLL 4 Hz,
# pull_in_time_s 0).  The pull-in transitory cannot end before one whole second
# (pull_in_span = (pull_in_time_s + 1) * (int)fs) and this satellite's bit
# synchronisation falls at call 1158, so 1250 calls pass through pull-in, the
# hand-over from FLL to PLL, bit sync and some of state 4.
FS = 2.0e6
NITEMS = 2000
SAT = synth.Satellite(7, 1234.5, 300.3, 45.0, 0.7, preamble_every_bits=25, code_doppler=True)
SIGNAL_S = 1.3
N_CALLS = 1250
NOISE_START = (3, 100.0, 500.0)  # PRN, code start sample, Doppler of a start on noise alone

# a. one override set per case: locked throughout, one bit sync, state 4 at the end
OPTION_CASES = [
    dict(pll_filter_order=2),
    dict(dll_filter_order=1),
    dict(dll_filter_order=3),
    dict(enable_fll_pull_in=1),
    dict(enable_fll_pull_in=1, pll_filter_order=2),
    dict(enable_fll_steady_state=1, fll_bw_hz=4),
    dict(enable_fll_pull_in=1, enable_fll_steady_state=1, fll_bw_hz=4),
    dict(carrier_aiding=0),
    dict(cn0_samples=7),
    dict(cn0_samples=63),
    dict(cn0_samples=64),
]

# c. the FLL stays on through the second second; 2.3 s of the same satellite
PULL_IN_CASE = dict(overrides=dict(pull_in_time_s=1, enable_fll_pull_in=1), seconds=2.3, calls=2290, sync_call=2158)

# d. losses the detectors reach on their own: input, overrides, the call index and the
# state of the loss in the free-running oracle, and whether the run passed state 3
LOSS_CASES = [
    ("noise", dict(max_carrier_lock_fail=50), 1049, 2, False),
    ("noise", dict(cn0_min=35, max_code_lock_fail=10), 1009, 2, False),
    ("noise", dict(carrier_lock_th=0.99, max_carrier_lock_fail=3), 1002, 2, False),
    ("signal", dict(bit_synchronization_time_limit_s=0), 999, 2, False),
    ("signal+noise0.5", dict(max_carrier_lock_fail=50), 1534, 4, False),
    ("signal+noise0.5", dict(cn0_min=38, max_code_lock_fail=20), 1631, 4, False),
    ("signal+noise1.2", dict(extend_correlation_symbols=10, max_carrier_lock_fail=3,
                             carrier_lock_test_smoother_alpha=0.2, carrier_lock_test_smoother_samples=5),
     1438, 4, True),
    ("signal+noise1.2", dict(extend_correlation_symbols=10, cn0_min=38, max_code_lock_fail=3,
                             cn0_smoother_alpha=0.2), 1208, 4, True),
]
LOSS_MARGIN = 5  # calls between the GPU's loss and the free-running oracle's: the counters step by one per call


# dll_filter_order = 3: Tracking_loop_filter's order-3 form is a double integrator in
# float (outputs 2 * y[n-1] - y[n-2]) fed c0 * x[n] + c1 * x[n-1] + c2 * x[n-2] with
# c = (12.3, -24.5, 12.2): every rounding of that sum, and every last-place
# difference between the device's and the host's discriminator output, is integrated
# twice and never decays, so two float evaluations drift apart over the calls.  The
# listed 1e-4 of code_freq_chips and rem_code_phase_samples cannot hold for it.
# Measured on the free-running oracle (lf3_float_vs_f64, pinned by
# test_oracle_tracking.py::test_order3_code_filter_float_drift), 1250 calls of the
# scenario signal: its float filter output lies 7.548e-4 chips/s from the same
# recursion in float64 on the same inputs, and the code periods that follow from
# the two sum to 1.248e-3 samples of code phase.  The bounds are twice those.
DLL3_FLOAT_VS_F64 = {"code_freq_chips": 7.548e-4, "rem_code_phase_samples": 1.248e-3}
DLL3_BOUNDS = {f: 2.0 * d for f, d in DLL3_FLOAT_VS_F64.items()}


def lf3_coefficients(bw, T):
    """Tracking_loop_filter::update_coefficients, order 3 without the last
    integrator (tracking_loop_filter.cc:98-197): float gains, double literals."""
    f32 = np.float32
    wn = f32(f32(bw) / f32(0.7845))
    g1, g2, g3 = float(f32(f32(wn * wn) * wn)), float(f32(f32(f32(1.1) * wn) * wn)), float(f32(f32(2.4) * wn))
    T = float(f32(T))
    return [f32(g3 + T / 2.0 * (g2 + T / 2.0 * g1)), f32(g1 * T * T / 2.0 - 2.0 * g3),
            f32(g3 + T / 2.0 * (-g2 + T / 2.0 * g1))]


def lf3_apply(x, coef, dtype):
    """Tracking_loop_filter::apply (:58-93) of that filter over the inputs x from a
    zero state, every product and sum rounded to dtype, in the reference's order."""
    c = [dtype(v) for v in coef]
    o1 = o2 = x1 = x2 = dtype(0)
    out = np.empty(len(x), np.float64)
    for k, v in enumerate(x):
        v = dtype(v)
        r = dtype(dtype(0) + dtype(dtype(2) * o1))
        r = dtype(r + dtype(dtype(-1) * o2))
        r = dtype(r + dtype(c[0] * v))
        r = dtype(r + dtype(c[1] * x1))
        r = dtype(r + dtype(c[2] * x2))
        o2, o1, x2, x1 = o1, r, x1, v
        out[k] = r
    return out


def lf3_float_vs_f64(recs, bw=4.0, T=0.001):
    """The order-3 code filter of a run's records (its inputs code_error_chips, its
    outputs code_error_filt_chips; one loop update per call, constant coefficients):
    (distance of the float recursion to the records' outputs -- 0 when the records
    are that recursion bit for bit; distance of the records' outputs to the float64
    recursion on the same inputs; the code phase, in samples, that the code periods
    1023 / code_freq * fs of the two accumulate)."""
    coef = lf3_coefficients(bw, T)
    filt = recs["code_error_filt_chips"].astype(np.float64)
    r32 = lf3_apply(recs["code_error_chips"], coef, np.float32)
    r64 = lf3_apply(recs["code_error_chips"], coef, np.float64)
    cf32 = recs["code_freq_chips"]
    cf64 = cf32 + (filt - r64)  # code_freq = chip rate - filter output (+ carrier aiding)
    drem = np.abs(np.cumsum(1023.0 / cf64 * FS - 1023.0 / cf32 * FS))
    return float(np.max(np.abs(r32 - filt))), float(np.max(np.abs(filt - r64))), float(drem.max())


# e. the restart after a loss: table row 5's input, then RESTART_SAT from the stamp of
# the second acquisition on
RESTART_SAT = synth.Satellite(12, -2200.0, 77.7, 47.0, 1.1, code_doppler=True)
RESTART_CALLS = 300
BESIDE_SAT = synth.Satellite(20, 2990.0, 640.4, 46.0, 2.1, preamble_every_bits=25, code_doppler=True)
RESTART_HD = dict(high_dyn=1, smoother_length=3)


@functools.lru_cache(maxsize=None)
def restart_input(beside):
    """Table row 5's input (the signal, then 0.5 s of noise) followed by RESTART_SAT,
    whose signal begins at the stamp of the second acquisition: (iq, that stamp).
    beside: BESIDE_SAT, noise-free, added over the whole length for a second channel."""
    head, _, _ = scenario_input("signal+noise0.5")
    tail = synth.gps_l1_iq(FS, (RESTART_CALLS + 20) * 2000, [RESTART_SAT], seed_offset=6)
    iq = np.concatenate([head, tail])
    if beside:
        iq = iq + synth.gps_l1_iq(FS, len(iq), [BESIDE_SAT], seed_offset=0, noise=False)
    iq.setflags(write=False)
    return iq, len(head)


# high_dyn: the rate steps are differences of the Doppler (and code frequency) steps
# over the 2 * smoother_length histories, computed in double from the float output
# of the carrier filter.  _replay_check wants them bit-identical, which holds only
# while the replayed Doppler is; it allows the Doppler itself 1e-2 Hz.  On the
# restarted run one call's Doppler comes out one float ulp (2.44e-4 Hz at 2200 Hz)
# from the host's -- a last-place difference of atan2f or of the float filter -- and
# sits in the histories for six calls, whose rates differ by 4.26e-14 rad/sample^2
# (1.3e-4 of a typical 1.5e-9) and 4.4e-18 chips/sample^2.  Measured on the
# free-running oracle of that run (hd_rates_float_vs_f64, pinned by
# test_oracle_tracking.py::test_high_dynamics_rate_float_sensitivity): the rates that
# follow from its float PLL filter lie 1.468e-13 rad/sample^2 from those of the same
# filter in float64 on the same discriminator outputs; through the carrier aiding
# (chip rate / carrier frequency / 2 pi) that is 1.517e-17 chips/sample^2.  The bounds
# are twice those.
HD_RESTART_FLOAT_VS_F64 = {"carrier_rate": 1.468e-13, "code_rate": 1.517e-17}
HD_RESTART_BOUNDS = {f: 2.0 * d for f, d in HD_RESTART_FLOAT_VS_F64.items()}


def pll3_apply(pll_hz, acq_doppler_hz, pll_bw_hz, T, dtype):
    """Tracking_FLL_PLL_filter, order 3, PLL only (tracking_FLL_PLL_filter.cc:61-74
    initialize, get_carrier_error with a zero FLL term) over the discriminator
    outputs pll_hz: the carrier Doppler per call, every operation rounded to dtype,
    the float parameters of set_params."""
    f32 = np.float32
    w0p = f32(f32(pll_bw_hz) / f32(0.7845))
    w0p2 = f32(w0p * w0p)
    k_w, k_x, k_e = dtype(f32(w0p2 * w0p)), dtype(f32(f32(1.1) * w0p2)), dtype(f32(f32(2.4) * w0p))
    t, half, zero = dtype(f32(T)), dtype(0.5), dtype(0)
    x, w = dtype(f32(2.0) * f32(acq_doppler_hz)), zero
    out = np.empty(len(pll_hz), np.float64)
    for k, p in enumerate(pll_hz):
        p = dtype(p)
        w = dtype(w + dtype(t * dtype(dtype(k_w * p) + zero)))
        x = dtype(x + dtype(t * dtype(dtype(dtype(half * w) + zero) + dtype(k_x * p))))
        out[k] = dtype(dtype(half * x) + dtype(k_e * p))
    return out


def hd_carrier_rates(doppler_hz, samples, L):
    """The carrier rate step of update_tracking_vars (dll_pll_veml_tracking.cc:1232-1251)
    per call, from the Doppler after each call's loop update and the length in
    samples the same update sets: mean of the newest L steps minus mean of the L
    before, over the newest L lengths, summed in the reference's order."""
    steps = TWO_PI * np.asarray(doppler_hz, np.float64) / FS
    out = np.zeros(len(steps))
    for k in range(2 * L - 1, len(steps)):
        cp1 = cp2 = total = 0.0
        for j in range(L):
            cp1 += steps[k - 2 * L + 1 + j]
            cp2 += steps[k - j]
            total += samples[k - j]
        out[k] = (cp2 / L - cp1 / L) / total
    return out


def hd_rates_float_vs_f64(recs, acq_doppler_hz, L, pll_bw_hz=40.0, T=0.001):
    """For a high_dyn run in state 2 (one PLL update per call): (distance of the float
    filter model to the records' Doppler, count of rate steps the model misses -- both
    0 when the records are that arithmetic bit for bit; distance between the carrier
    rates that follow from the float filter and from the float64 one; the same for
    the code rates, which the Doppler reaches through the carrier aiding)."""
    e32 = pll3_apply(recs["carr_phase_error_hz"], acq_doppler_hz, pll_bw_hz, T, np.float32)
    e64 = pll3_apply(recs["carr_phase_error_hz"], acq_doppler_hz, pll_bw_hz, T, np.float64)
    samples = recs["consumed"][1:].astype(np.float64)  # the length a call's update sets is the next call's
    n = len(samples)
    r32, r64 = hd_carrier_rates(e32[:n], samples, L), hd_carrier_rates(e64[:n], samples, L)
    d = float(np.max(np.abs(r32 - r64)))
    return (float(np.max(np.abs(e32 - recs["carrier_doppler_hz"]))),
            int(np.count_nonzero(r32.astype(np.float32) != recs["carrier_rate"][:n])), d,
            d * 1.023e6 / 1.57542e9 / TWO_PI)


def case_id(overrides):
    return ",".join("%s=%g" % kv for kv in overrides.items())


@functools.lru_cache(maxsize=None)
def _signal(seconds):
    iq = synth.gps_l1_iq(FS, int(seconds * FS), [SAT], seed_offset=5)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def _noise(seconds):
    iq = synth.gps_l1_iq(FS, int(seconds * FS), [], seed_offset=9)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def scenario_input(name):
    """(iq, noise_spans, (prn, code start sample, Doppler)) of a named input; the
    arrays are shared between the tests and read-only."""
    sat_start = (SAT.prn,) + _acq(SAT, FS)
    if name == "noise":
        return _noise(SIGNAL_S), ((0, len(_noise(SIGNAL_S))),), NOISE_START
    if name == "signal":
        return _signal(SIGNAL_S), (), sat_start
    if name == "signal_long":
        return _signal(PULL_IN_CASE["seconds"]), (), sat_start
    head, tail = name.split("+noise")
    assert head == "signal", name
    sig = _signal(SIGNAL_S)
    iq = np.concatenate([sig, _noise(float(tail))])
    iq.setflags(write=False)
    return iq, ((len(sig), len(iq)),), sat_start


def scenario_conf(overrides, base=None):
    """_conf(FS) (or a copy of base) with one case's overrides."""
    c = _conf(FS) if base is None else base.copy()
    for k, v in overrides.items():
        c[k] = v
    return c


def oracle_free_run(name, overrides, calls):
    """The free-running oracle on a named input: (records, first sample, channel)."""
    iq, _, (prn, delay, dop) = scenario_input(name)
    ch = trk.Channel(scenario_conf(overrides)[0:1].view(trk.TRK_CONF_DTYPE))
    first = ch.start(synth.gps_ca_chips(prn), delay, dop, 0, NITEMS)
    recs, _ = ch.run(iq, 0, first, calls)
    return recs, first, ch

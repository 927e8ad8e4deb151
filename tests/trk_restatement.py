"""numpy restatement of dll_pll_veml_tracking::general_work, states 2-4 (not a test module).

oracle/trk_oracle.c stops at BeiDou B1I and is not to be extended, so the loop of the
Galileo E5a (5X) and GPS L5 rows is checked against this file.  It follows
src/algorithms/tracking/gnuradio_blocks/dll_pll_veml_tracking.cc of the reference:
the constructor's signal table (:170-430), start_tracking (:640-882),
acquire_secondary (:923-967), cn0_and_tracking_lock_status (:970-1056), run_dll_pll
(:1092-1179), update_tracking_vars (:1216-1287), save_correlation_results
(:1288-1400) and the state machine of general_work (:1784-2152), with the loop
libraries it calls (tracking_loop_filter.cc, tracking_FLL_PLL_filter.cc,
tracking_discriminators.cc, lock_detectors.cc, exponential_smoother.cc).  numpy
float32 stands where the reference computes in float and Python float (float64) where
it computes in double.  high_dyn is not restated.

test_trk_restatement.py pins it against the C oracle on the three signals both know;
it is trusted only for the constructor rows it adds.

Channel mirrors oracle.trk.Channel: start(), run() (free running, correlating with
oracle/volk.py's multicorrelator) and replay() (taps in, records out).
"""
import math

import numpy as np

from oracle import trk, volk

f32 = np.float32
PI = 3.1415926535898  # GNSS_PI (MATH_CONSTANTS.h:47-50)
TWO_PI = 2.0 * PI
HALF_PI = PI / 2.0

GPS_1C, GAL_1B, BDS_B1, GAL_5X, GPS_L5 = 0, 1, 2, 3, 4
F_VALID_OUTPUT, F_LOSS_OF_LOCK, F_PLL_180, F_BIT_SYNC, F_LOGGED = 1, 2, 4, 8, 32

GPS_CA_PREAMBLE = "1" * 20 + "0" * 60 + "1" * 20 + "0" * 20 + "1" * 40  # GPS_L1_CA.h:61-73, 160 symbols
GAL_E1C_SECONDARY = "0011100000001010110110010"
BDS_B1I_NH = "00000100110101001110"
BDS_GEO_PREAMBLE = "1111110000001100001100"
GAL_E5A_I_SECONDARY = "10000100001011101001"  # Galileo_E5a.h:3581
GPS_L5I_NH = "0000110101"                     # GPS_L5.h:171
GPS_L5Q_NH = "00000100110101001110"           # GPS_L5.h:172


def _c(re=0.0, im=0.0):
    return [f32(re), f32(im)]


def _hypot(a):
    return f32(np.hypot(a[0], a[1]))


class _LoopFilter:
    """Tracking_loop_filter without the last integrator (tracking_loop_filter.cc:58-197)."""

    def __init__(self, T, bw, order):
        self.T, self.bw, self.order = f32(T), f32(bw), order
        self.inputs = [f32(0)] * 4
        self.outputs = [f32(0)] * 4
        self.idx = 0
        self.update()

    def update(self):
        T = float(self.T)
        if self.order == 1:
            self.icoef, self.ocoef = [f32(self.bw * f32(4.0))], []
        elif self.order == 2:
            zeta = f32(1.0) / np.sqrt(f32(2.0))
            wn = f32(f32(self.bw * f32(f32(8.0) * zeta)) / f32(f32(f32(f32(4.0) * zeta) * zeta) + f32(1.0)))
            g1 = f32(wn * wn)
            g2 = float(f32(f32(wn * f32(2.0)) * zeta))
            g1T = float(f32(g1 * self.T))  # float product, then double (g1 * T / 2.0)
            self.icoef = [f32(g1T / 2.0 + g2), f32(g1T / 2.0 - g2)]
            self.ocoef = [f32(1.0)]
        else:
            wn = f32(self.bw / f32(0.7845))
            g1f = f32(f32(wn * wn) * wn)
            g1 = float(g1f)
            g2 = float(f32(f32(f32(1.1) * wn) * wn))
            g3 = float(f32(f32(2.4) * wn))
            g1TT = float(f32(f32(g1f * self.T) * self.T))  # g1 * T * T in float
            self.icoef = [f32(g3 + T / 2.0 * (g2 + T / 2.0 * g1)), f32(g1TT / 2.0 - 2.0 * g3),
                          f32(g3 + T / 2.0 * (-g2 + T / 2.0 * g1))]
            self.ocoef = [f32(2.0), f32(-1.0)]

    def initialize(self, v):
        self.inputs = [f32(0)] * 4
        self.outputs = [f32(v)] * 4
        self.idx = 3

    def apply(self, x):
        r = f32(0)
        for i, c in enumerate(self.ocoef):
            r = f32(r + f32(c * self.outputs[(self.idx + i) % 4]))
        self.idx = (self.idx - 1) % 4
        self.inputs[self.idx] = f32(x)
        for i, c in enumerate(self.icoef):
            r = f32(r + f32(c * self.inputs[(self.idx + i) % 4]))
        self.outputs[self.idx] = r
        return r


class _CarrierFilter:
    """Tracking_FLL_PLL_filter (tracking_FLL_PLL_filter.cc:23-101)."""

    def set_params(self, fll_bw, pll_bw, order):
        self.order = order
        fll_bw, pll_bw = f32(fll_bw), f32(pll_bw)
        self.a2 = f32(1.414)
        if order == 3:
            self.b3, self.a3 = f32(2.4), f32(1.1)
            self.w0p = f32(pll_bw / f32(0.7845))
            self.w0p2 = f32(self.w0p * self.w0p)
            self.w0p3 = f32(self.w0p2 * self.w0p)
            self.w0f = f32(fll_bw / f32(0.53))
            self.w0f2 = f32(self.w0f * self.w0f)
        else:
            self.w0p = f32(pll_bw / f32(0.53))
            self.w0p2 = f32(self.w0p * self.w0p)
            self.w0f = f32(fll_bw / f32(0.25))

    def initialize(self, doppler):
        if self.order == 3:
            self.x, self.w = f32(f32(2.0) * f32(doppler)), f32(0)
        else:
            self.w, self.x = f32(doppler), f32(0)

    def error(self, fll, pll, t):
        fll, pll, t = f32(fll), f32(pll), f32(t)
        if self.order == 3:
            self.w = f32(self.w + f32(t * f32(f32(self.w0p3 * pll) + f32(self.w0f2 * fll))))
            self.x = f32(self.x + f32(t * f32(f32(f32(f32(0.5) * self.w) + f32(f32(self.a2 * self.w0f) * fll)) +
                                              f32(f32(self.a3 * self.w0p2) * pll))))
            return f32(f32(f32(0.5) * self.x) + f32(f32(self.b3 * self.w0p) * pll))
        w_new = f32(f32(self.w + f32(f32(pll * self.w0p2) * t)) + f32(f32(fll * self.w0f) * t))
        e = f32(f32(f32(0.5) * f32(w_new + self.w)) + f32(f32(self.a2 * self.w0p) * pll))
        self.w = w_new
        return e


class _Smoother:
    """Exponential_Smoother (exponential_smoother.cc:23-110)."""

    def __init__(self, alpha, min_value, offset, samples):
        a = f32(min(max(float(alpha), 0.0), 1.0))
        self.alpha, self.one_minus = a, f32(f32(1.0) - a)
        self.min_value, self.offset = f32(min_value), f32(offset)
        self.samples = max(1, int(samples))
        self.old = f32(0)
        self.reset()

    def reset(self):
        self.initializing, self.counter, self.buf = True, 0, []

    def smooth(self, raw):
        raw = f32(raw)
        if not self.initializing:
            self.old = f32(f32(self.alpha * raw) + f32(self.one_minus * self.old))
            return self.old
        self.counter += 1
        self.buf.append(raw)
        if self.counter == self.samples:
            acc = f32(0)
            for v in self.buf:
                acc = f32(acc + v)
            self.old = f32(acc / f32(len(self.buf)))
            if self.old < f32(self.min_value + self.offset):
                self.counter, self.buf = 0, []
            else:
                self.initializing = False
        return raw


def _phase_unwrap(p):
    if p >= HALF_PI:
        return p - PI
    if p <= -HALF_PI:
        return p + PI
    return p


def _atan_ratio(v):
    with np.errstate(all="ignore"):
        return np.arctan(f32(v[1] / v[0]))


def _cn0_m2m4(buf, n, coh):
    """cn0_m2m4_estimator (lock_detectors.cc:90-120)."""
    psig = m2 = m4 = f32(0)
    for re, im in buf[:n]:
        psig = f32(psig + np.abs(re))
        aux = f32(f32(im * im) + f32(re * re))
        m2 = f32(m2 + aux)
        m4 = f32(m4 + f32(aux * aux))
    nf = f32(n)
    psig = f32(psig / nf)
    psig = f32(psig * psig)
    m2, m4 = f32(m2 / nf), f32(m4 / nf)
    with np.errstate(all="ignore"):
        aux = np.sqrt(f32(f32(f32(f32(2.0) * m2) * m2) - m4))
        snr = f32(psig / f32(m2 - psig)) if np.isnan(aux) else f32(aux / f32(m2 - aux))
        return f32(f32(f32(10.0) * np.log10(snr)) - f32(f32(10.0) * np.log10(f32(coh))))


class Channel:
    """One dll_pll_veml_tracking channel; conf: a one-element TRK_CONF_DTYPE array.
    secondary_code: the PRN's E5a-Q secondary code ('0'/'1'), 5X pilot tracking only."""

    def __init__(self, conf, secondary_code=None):
        p = {k: conf[k][0].item() for k in conf.dtype.names}
        if p["high_dyn"]:
            raise ValueError("high_dyn is not restated")
        self.p = p
        sig = p["signal"]
        self.veml = False
        self.data_sec = ""
        self.interchange_iq = False
        self.spc_chip = 1
        if sig == GPS_1C:  # :170-191
            self.carrier_hz, self.period, self.chip_rate, self.length = 1.57542e9, 0.001, 1.023e6, 1023
            self.secondary, p["track_pilot"] = False, 0
            self.sec, self.symbols_per_bit = GPS_CA_PREAMBLE, 20
        elif sig == GAL_1B:  # :258-290
            self.carrier_hz, self.period, self.chip_rate, self.length = 1.57542e9, 0.004, 1.023e6, 4092
            self.symbols_per_bit, self.spc_chip, self.veml = 1, 2, True
            self.secondary = bool(p["track_pilot"])
            self.sec = GAL_E1C_SECONDARY if self.secondary else ""
        elif sig == BDS_B1:  # :391-411
            self.carrier_hz, self.period, self.chip_rate, self.length = 1.561098e9, 0.001, 2.046e6, 2046
            self.symbols_per_bit, self.secondary, p["track_pilot"] = 20, True, 0
            self.sec = self.data_sec = BDS_B1I_NH
        elif sig == GAL_5X:  # :289-319
            self.carrier_hz, self.period, self.chip_rate, self.length = 1.17645e9, 0.001, 1.023e7, 10230
            self.symbols_per_bit, self.secondary = 20, True
            if p["track_pilot"]:
                if secondary_code is None:
                    raise ValueError("5X pilot tracking needs the PRN's secondary code")
                self.sec, self.data_sec, self.interchange_iq = str(secondary_code), GAL_E5A_I_SECONDARY, True  # :703
            else:
                self.sec = GAL_E5A_I_SECONDARY
        elif sig == GPS_L5:  # :210-244
            self.carrier_hz, self.period, self.chip_rate, self.length = 1.17645e9, 0.001, 1.023e7, 10230
            self.symbols_per_bit, self.secondary = 10, True
            if p["track_pilot"]:
                self.sec, self.data_sec = GPS_L5Q_NH, GPS_L5I_NH
            else:
                self.sec, self.interchange_iq = GPS_L5I_NH, True
        else:
            raise ValueError("signal %d" % sig)
        self.track_pilot = bool(p["track_pilot"])
        self.enable_ext = p["extend_correlation_symbols"] > 1  # :511-520
        if not self.enable_ext:
            p["extend_correlation_symbols"] = 1
        if p["vector_length"] == 0:
            p["vector_length"] = int(round(p["fs_in"] / (self.chip_rate / self.length)))
        self.fs = p["fs_in"]
        self.n_taps = 5 if self.veml else 3
        self.iE, self.iP, self.iL = (1, 2, 3) if self.veml else (0, 1, 2)
        self.spc = f32(p["early_late_space_chips"])
        self.code_freq = self.chip_rate
        self.code_filter = _LoopFilter(self.period, p["dll_bw_hz"], p["dll_filter_order"])
        self.carrier_filter = _CarrierFilter()
        self.carrier_filter.set_params(p["fll_bw_hz"], p["pll_bw_hz"], p["pll_filter_order"])
        self.cn0_smoother = _Smoother(p["cn0_smoother_alpha"], 25.0, 12.0,
                                      p["cn0_smoother_samples"] // int(self.period * 1000.0))
        self.lock_smoother = _Smoother(p["carrier_lock_test_smoother_alpha"], -1.0, 0.0,
                                       p["carrier_lock_test_smoother_samples"])
        self.state = 0
        self.flag_pll_180 = False
        self.taps = [_c() for _ in range(5)]
        self.prompt_data = _c()
        self.VE = self.E = self.P = self.L = self.VL = self.P_old = self.P_data = _c()
        self.current_prn_length_samples = 0
        self.rem_carr = f32(0)
        self.carrier_phase_rate_step = self.code_phase_rate_step = 0.0
        self.errs = [0.0] * 4  # carr_phase_error_hz, carr_error_filt_hz, code_error_chips, code_error_filt_chips
        self.carrier_doppler = self.acc_carrier_phase = self.rem_code_samples = 0.0
        self.cn0 = self.evm = 0.0
        self.lock_test = 1.0

    @property
    def vector_length(self):
        return self.p["vector_length"]

    def _set_shifts(self, narrow):
        p, s = self.p, f32(self.spc_chip)
        el = f32(p["early_late_space_narrow_chips" if narrow else "early_late_space_chips"])
        vel = f32(p["very_early_late_space_narrow_chips" if narrow else "very_early_late_space_chips"])
        self.shifts = np.array([-vel * s, -el * s, 0.0, el * s, vel * s] if self.veml else [-el * s, 0.0, el * s], f32)

    def _clear_tracking_vars(self):  # :1192-1213
        self.taps = [_c() for _ in range(5)]
        if self.track_pilot:
            self.prompt_data, self.P_data = _c(), _c()
        self.P_old = _c()
        self.errs = [0.0] * 4
        self.current_symbol = self.current_data_symbol = 0
        self.circ = []
        self.carrier_phase_rate_step = self.code_phase_rate_step = 0.0

    def start(self, code, acq_delay_samples, acq_doppler_hz, acq_samplestamp, nitems_read, prn=1, data_code=None):
        """start_tracking (:640-882) and the state-1 pull-in call (:1813-1844)."""
        p = self.p
        self.code = np.ascontiguousarray(code, f32)
        self.data_code = None if data_code is None else np.ascontiguousarray(data_code, f32)
        if self.track_pilot and self.data_code is None:
            raise ValueError("pilot tracking needs the data replica")
        self.extend = p["extend_correlation_symbols"]
        self.extend_count = 0
        if p["signal"] == BDS_B1:
            if 0 < prn < 6 or prn > 58:  # GEO, D2 (:762-778)
                self.extend = min(self.extend, 2)
                self.symbols_per_bit, self.secondary, self.sec, self.data_sec = 2, False, BDS_GEO_PREAMBLE, ""
            else:  # D1 (:779-795)
                self.symbols_per_bit, self.secondary, self.sec, self.data_sec = 20, True, BDS_B1I_NH, BDS_B1I_NH
        self.acq_stamp = int(acq_samplestamp)
        self.carrier_doppler = float(acq_doppler_hz)
        self.carrier_phase_step = TWO_PI * self.carrier_doppler / self.fs
        self.carrier_phase_rate_step = 0.0
        self.taps = [_c() for _ in range(5)]
        self.carrier_lock_fail = self.code_lock_fail = 0
        self.rem_code_samples = self.rem_code_chips = self.acc_carrier_phase = 0.0
        self.rem_carr = f32(0)
        self.cn0_counter = 0
        self.lock_test, self.cn0, self.evm = 1.0, 0.0, 0.0
        self._set_shifts(False)
        self.prompt_data = _c()
        self.corr_time = self.period
        self.carrier_filter.set_params(p["fll_bw_hz"], p["pll_bw_hz"], p["pll_filter_order"])
        self.code_filter.bw = f32(p["dll_bw_hz"])
        self.code_filter.update()
        self.code_filter.T = f32(self.period)
        self.code_filter.update()
        self.carrier_filter.initialize(f32(acq_doppler_hz))
        self.code_filter.initialize(0.0)
        self.cloop, self.pull_in, self.circ, self.acc_init = True, True, [], False
        self.prompt_buffer = [_c() for _ in range(p["cn0_samples"])]
        # state 1
        delta = float(int(nitems_read) - self.acq_stamp) - float(acq_delay_samples)
        self.code_freq = self.chip_rate
        self.code_phase_step = self.code_freq / self.fs
        self.code_phase_rate_step = 0.0
        T_prn_samples = (1.0 / self.code_freq) * float(self.length) * self.fs
        acq_phase = T_prn_samples - math.fmod(delta, T_prn_samples)
        self.current_prn_length_samples = int(math.floor(T_prn_samples + 0.5))  # round(), positive arguments
        off = int(math.floor(acq_phase + 0.5))
        self.acc_carrier_phase -= self.carrier_phase_step * float(off)
        self.state = 2
        self.cn0_smoother.reset()
        self.lock_smoother.reset()
        self.current_symbol = self.current_data_symbol = 0
        return int(nitems_read) + off

    def force_loss_of_lock(self):  # msg_handler_telemetry_to_trk (:614-637)
        self.carrier_lock_fail = 200000

    # ------------------------------------------------------------ the pieces of a call
    def _correlate(self, x):  # do_correlation_step (:1064-1089)
        s = f32(self.spc_chip)
        args = (float(self.rem_carr), float(f32(self.carrier_phase_step)), float(f32(f32(self.rem_code_chips) * s)),
                float(f32(f32(self.code_phase_step) * s)), self.vector_length)
        out = volk.multicorrelator_real_codes_avx(x, self.code, self.shifts, *args)
        self.taps = [_c(v.real, v.imag) for v in out] + [_c() for _ in range(5 - len(out))]
        if self.track_pilot:
            d = volk.multicorrelator_real_codes_avx(x, self.data_code, self.shifts[self.iP:self.iP + 1], *args)
            self.prompt_data = _c(d[0].real, d[0].imag)

    def _cn0_and_lock(self, coh):  # :970-1056
        n = self.p["cn0_samples"]
        if self.cn0_counter < n:
            self.prompt_buffer[self.cn0_counter] = list(self.P)
            self.cn0_counter += 1
            return True
        self.prompt_buffer[self.cn0_counter % n] = list(self.P)
        self.cn0_counter += 1
        self.cn0 = float(self.cn0_smoother.smooth(_cn0_m2m4(self.prompt_buffer, n, coh)))
        si, sq = f32(f32(0) + self.prompt_buffer[0][0]), f32(f32(0) + self.prompt_buffer[0][1])  # detector over 1 element
        with np.errstate(all="ignore"):
            test = f32(f32(f32(si * si) - f32(sq * sq)) / f32(f32(si * si) + f32(sq * sq)))
        self.lock_test = float(self.lock_smoother.smooth(test))
        if not self.pull_in:
            if self.lock_test < self.p["carrier_lock_th"]:
                self.carrier_lock_fail += 1
            elif self.carrier_lock_fail > 0:
                self.carrier_lock_fail -= 1
            if self.cn0 < self.p["cn0_min"]:
                self.code_lock_fail += 1
            elif self.code_lock_fail > 0:
                self.code_lock_fail -= 1
        if self.carrier_lock_fail > self.p["max_carrier_lock_fail"] or self.code_lock_fail > self.p["max_code_lock_fail"]:
            self.carrier_lock_fail = self.code_lock_fail = 0
            return False
        s = f32(0)  # EVM (:1027-1053)
        for re, _ in self.prompt_buffer:
            s = f32(s + f32(re * re))
        with np.errstate(all="ignore"):
            d = np.sqrt(f32(s / f32(n)))
            s = f32(0)
            for re, im in self.prompt_buffer:
                a = f32(np.abs(f32(re / d)) - f32(1))
                b = f32(np.abs(f32(im / d)) - f32(0))
                s = f32(f32(s + f32(a * a)) + f32(b * b))
            self.evm = math.sqrt(float(f32(f32(s / f32(n)) / f32(1))))
        return True

    def _run_dll_pll(self):  # :1092-1179
        p = self.p
        if self.cloop:
            ph = float(_atan_ratio(self.P)) if self.P[0] != 0 else 0.0
        else:
            ph = float(np.arctan2(self.P[1], self.P[0]))
        ph /= TWO_PI
        t = f32(self.corr_time)
        if (self.pull_in and p["enable_fll_pull_in"]) or p["enable_fll_steady_state"]:
            d = float(f32(_atan_ratio(self.P) - _atan_ratio(self.P_old)))
            if math.isnan(d):
                d = 0.0
            fe = _phase_unwrap(d) / (self.corr_time - 0.0) / TWO_PI
            self.P_old = list(self.P)
            if self.pull_in and p["enable_fll_pull_in"]:
                filt = float(self.carrier_filter.error(f32(fe), f32(0), t))
            else:
                filt = float(self.carrier_filter.error(f32(fe), f32(ph), t))
        else:
            filt = float(self.carrier_filter.error(f32(0), f32(ph), t))
        self.carrier_doppler = filt
        if self.veml:
            # float products summed in float, the square root in double (:139-149)
            early = math.sqrt(float(f32(f32(f32(f32(self.VE[0] * self.VE[0]) + f32(self.VE[1] * self.VE[1])) +
                                            f32(self.E[0] * self.E[0])) + f32(self.E[1] * self.E[1]))))
            late = math.sqrt(float(f32(f32(f32(f32(self.L[0] * self.L[0]) + f32(self.L[1] * self.L[1])) +
                                           f32(self.VL[0] * self.VL[0])) + f32(self.VL[1] * self.VL[1]))))
            code_err = 0.0 if early + late == 0.0 else (early - late) / (early + late)
        else:
            pe, pl = float(_hypot(self.E)), float(_hypot(self.L))
            slope = y = f32(1.0)
            code_err = 0.0 if pe + pl == 0.0 else float(f32(f32(y - f32(slope * self.spc)) / slope)) * (pe - pl) / (pe + pl)
        code_filt = float(self.code_filter.apply(f32(code_err)))
        self.code_freq = self.chip_rate - code_filt
        if p["carrier_aiding"]:
            self.code_freq += self.carrier_doppler * self.chip_rate / self.carrier_hz
        self.errs = [ph, filt, code_err, code_filt]

    def _update_tracking_vars(self):  # :1216-1287
        T_prn_samples = (1.0 / self.code_freq) * float(self.length) * self.fs
        K_blk = T_prn_samples + self.rem_code_samples
        self.current_prn_length_samples = int(math.floor(K_blk))
        self.carrier_phase_step = TWO_PI * self.carrier_doppler / self.fs
        n = float(self.current_prn_length_samples)
        adv = self.carrier_phase_step * n + 0.5 * self.carrier_phase_rate_step * n * n
        self.rem_carr = f32(self.rem_carr + f32(adv))
        self.rem_carr = f32(math.fmod(float(self.rem_carr), TWO_PI))
        self.acc_carrier_phase -= adv
        self.code_phase_step = self.code_freq / self.fs
        self.rem_code_samples = K_blk - n
        self.rem_code_chips = self.code_freq * self.rem_code_samples / self.fs

    def _acquire_secondary(self):  # :923-967
        corr = 0
        for v, ch in zip(self.circ, self.sec):
            corr += (1 if ch == "0" else -1) if v < 0 else (-1 if ch == "0" else 1)
        if abs(corr) == len(self.sec):
            self.flag_pll_180 = corr < 0
            return True
        return False

    @staticmethod
    def _cadd(a, b, positive):
        return [f32(a[0] + b[0]), f32(a[1] + b[1])] if positive else [f32(a[0] - b[0]), f32(a[1] - b[1])]

    def _save_correlation_results(self):  # :1288-1400
        pos = True
        if self.secondary:
            pos = self.sec[self.current_symbol] == "0"
            self.current_symbol = (self.current_symbol + 1) % len(self.sec)
        if self.veml:
            self.VE = self._cadd(self.VE, self.taps[0], pos)
            self.VL = self._cadd(self.VL, self.taps[4], pos)
        self.E = self._cadd(self.E, self.taps[self.iE], pos)
        self.P = self._cadd(self.P, self.taps[self.iP], pos)
        self.L = self._cadd(self.L, self.taps[self.iL], pos)
        pd = self.prompt_data if self.track_pilot else self.taps[self.iP]
        if self.symbols_per_bit > 1:
            if len(self.data_sec) > 0:
                self.P_data = self._cadd(self.P_data, pd, self.data_sec[self.current_data_symbol] == "0")
                self.current_data_symbol = (self.current_data_symbol + 1) % len(self.data_sec)
            else:
                self.P_data = self._cadd(self.P_data, pd, True)
                self.current_data_symbol = (self.current_data_symbol + 1) % self.symbols_per_bit
        else:
            self.P_data = list(pd)
        self.cloop = not self.track_pilot

    def _log(self, r):  # log_data (:1403-1500)
        r["flags"] |= F_LOGGED
        r["log_accu"] = [_hypot(self.VE) if self.veml else 0.0, _hypot(self.E), _hypot(self.P), _hypot(self.L),
                         _hypot(self.VL) if self.veml else 0.0]

    def _output(self, r):  # :2000-2017, :2054-2063
        re, im = float(self.P_data[0]), float(self.P_data[1])
        r["prompt_i"], r["prompt_q"] = (im, re) if self.interchange_iq else (re, im)
        r["flags"] |= F_VALID_OUTPUT
        self.P_data = _c()

    def call(self, x, taps, nitems_read, r):
        """One general_work call at nitems_read: x the call's samples, or taps the 12
        floats of a record (five complex tap slots and the data prompt).  False in standby."""
        p = self.p
        if self.state not in (2, 3, 4):
            return False
        r["sample_counter"], r["state"] = nitems_read, self.state
        lost = False
        elapsed = ((int(nitems_read) - self.acq_stamp) % (1 << 64)) // int(self.fs)  # :1794-1803, unsigned
        if self.pull_in and p["pull_in_time_s"] < elapsed:
            self.pull_in = False
            self.carrier_lock_fail = self.code_lock_fail = 0
        if taps is None:
            self._correlate(x)
        else:
            self.taps = [_c(taps[2 * k], taps[2 * k + 1]) if k < self.n_taps else _c() for k in range(5)]
            if self.track_pilot:
                self.prompt_data = _c(taps[10], taps[11])
        if self.state == 2:
            if self.veml:
                self.VE, self.VL = list(self.taps[0]), list(self.taps[4])
            self.E, self.P, self.L = list(self.taps[self.iE]), list(self.taps[self.iP]), list(self.taps[self.iL])
            self.spc = f32(p["early_late_space_chips"])
            if p["bit_synchronization_time_limit_s"] < elapsed:
                self.carrier_lock_fail = 300000
            if not self._cn0_and_lock(self.period):
                self._clear_tracking_vars()
                self.state, lost = 0, True
            else:
                self._run_dll_pll()
                self._update_tracking_vars()
                self._log(r)
                nxt = False
                if not self.pull_in:
                    if self.secondary or self.symbols_per_bit > 1:
                        self.circ.append(self.taps[self.iP][0])
                        self.circ = self.circ[-len(self.sec):]
                        if len(self.circ) == len(self.sec):
                            nxt = self._acquire_secondary()
                    else:
                        nxt = True
                if nxt:
                    self.VE, self.E, self.P, self.L, self.VL, self.P_data = _c(), _c(), _c(), _c(), _c(), _c()
                    self.circ = []
                    self.current_symbol = self.current_data_symbol = 0
                    r["flags"] |= F_BIT_SYNC
                    if self.enable_ext:  # :1945-1983
                        self.extend_count = 0
                        self.corr_time = float(f32(f32(self.extend) * f32(self.period)))
                        self.state = 3
                        self.code_filter.T = f32(self.corr_time)
                        self.code_filter.update()
                        self.code_filter.bw = f32(p["dll_bw_narrow_hz"])
                        self.code_filter.update()
                        self.carrier_filter.set_params(p["fll_bw_hz"], p["pll_bw_narrow_hz"], p["pll_filter_order"])
                        self._set_shifts(True)
                        self.spc = f32(p["early_late_space_narrow_chips"])
                    else:
                        self.state = 4
        elif self.state == 3:  # :1989-2026
            self._save_correlation_results()
            self._update_tracking_vars()
            if self.current_data_symbol == 0:
                self._log(r)
                self._output(r)
            self.extend_count += 1
            if self.extend_count == self.extend - 1:
                self.extend_count, self.state = 0, 4
        else:  # state 4 (:2028-2120)
            self._save_correlation_results()
            if not self._cn0_and_lock(self.period * float(self.extend)):
                self._clear_tracking_vars()
                self.state, lost = 0, True
            else:
                self._run_dll_pll()
                self._update_tracking_vars()
                if not self.acc_init:
                    self.acc_carrier_phase, self.acc_init = -float(self.rem_carr), True
                if self.current_data_symbol == 0:
                    self._log(r)
                    self._output(r)
                self.VE, self.E, self.P, self.L, self.VL = _c(), _c(), _c(), _c(), _c()
                if self.enable_ext:
                    self.state = 3
        t = r["taps"]
        for k in range(self.n_taps):
            t[2 * k], t[2 * k + 1] = self.taps[k]
        r["data_prompt"] = self.prompt_data
        r["carrier_rate"], r["code_rate"] = self.carrier_phase_rate_step, self.code_phase_rate_step
        (r["carr_phase_error_hz"], r["carr_error_filt_hz"], r["code_error_chips"],
         r["code_error_filt_chips"]) = self.errs
        if lost:
            r["flags"] |= F_LOSS_OF_LOCK
        if self.flag_pll_180:
            r["flags"] |= F_PLL_180
        r["consumed"] = self.current_prn_length_samples
        r["rem_carr_phase_rad"] = self.rem_carr
        r["carrier_doppler_hz"], r["code_freq_chips"] = self.carrier_doppler, self.code_freq
        r["rem_code_phase_samples"], r["acc_carrier_phase_rad"] = self.rem_code_samples, self.acc_carrier_phase
        r["cn0_db_hz"], r["carrier_lock_test"], r["evm"] = self.cn0, self.lock_test, self.evm
        return True

    def run(self, iq, iq_first_sample, first_sample, max_epochs):
        """Free running over iq (complex64, absolute index iq_first_sample) from first_sample."""
        iq = np.ascontiguousarray(iq, np.complex64)
        vl = self.vector_length
        recs = np.zeros(max_epochs, trk.TRK_EPOCH_DTYPE)
        n, k = first_sample, 0
        while k < max_epochs:
            off = n - iq_first_sample
            if off < 0 or off + vl > len(iq) or not self.call(iq[off:off + vl], None, n, recs[k]):
                break
            n += int(recs[k]["consumed"])
            k += 1
        return recs[:k], n

    def replay(self, records, force_before=()):
        """The loop on another implementation's correlator outputs, call by call at the
        same input positions; force_before: record indices before which a telemetry
        fault arrives.  Returns this channel's own records."""
        out = np.zeros(len(records), trk.TRK_EPOCH_DTYPE)
        force = set(int(i) for i in force_before)
        for k, rec in enumerate(records):
            if k in force:
                self.force_loss_of_lock()
            taps = np.concatenate([rec["taps"], rec["data_prompt"]]).astype(f32)
            if not self.call(None, taps, int(rec["sample_counter"]), out[k]):
                return out[:k]
        return out

"""numpy restatement of kf_tracking::general_work, states 2-4 (not a test module).

src/algorithms/tracking/gnuradio_blocks/kf_tracking.cc of the reference is
dll_pll_veml_tracking.cc with a four-state Kalman filter (code-phase error, carrier
phase, Doppler, Doppler rate) where that block has its two loop filters.  KfChannel
derives from trk_restatement.Channel and overrides what differs:

  init_kf (:857-895) in the state-1 pull-in call (:1824), i.e. in start();
  run_Kf (:1129-1204) in run_dll_pll's place, after update_kf_cn0 (:938-955) in state 4;
  update_kf_narrow_integration_time (:898-935) at the switch to the extended
    correlator, before the taps and spc take their narrow values (:1943);
  update_tracking_vars (:1237-1313), which subtracts the *float* remnant from the
    accumulated carrier phase (:1279-1284);
  cn0_and_tracking_lock_status (:1036-1093), which has no EVM (restated whole, with
    the estimator's log10 correctly rounded);
  clear_tracking_vars (:1217-1233), which leaves the discriminator and filter outputs
    that log_data dumps (:1497-1504) alone.

Read side by side, the rest agrees with the DLL/PLL block and is inherited: the
pull-in and bit-synchronisation time limits (:1782-1790, :1853-1858), acquire_secondary,
save_correlation_results (:1316-1426), the outputs of states 3 and 4 (:1979-2002,
:2029-2053) and the state transitions.  The narrow loop-filter bandwidths the base class
sets at the switch act on filters this class never runs.

float64 numpy stands where the reference uses arma::mat / arma::vec, numpy float32 where
it uses float (the accumulators the discriminators read, d_rem_carr_phase_rad, the
remnant).  The float library calls whose result the filter keeps -- atan / atan2 and
hypot in the discriminators, log10 in the C/N0 that R is rebuilt from -- are evaluated
correctly rounded (in double, rounded to float), as the device's Kalman loop does: x(1)
never wraps and a replay feeds nothing back, so a last place that two libraries disagree
on would stay in x and P for good, and correct rounding is the one value both can give.  The reference cannot be built without Armadillo and GNU Radio and holds no
captured Kalman numbers, so this file is the reference of the device loop;
test_kf_restatement.py pins it by construction.

`variant="solve"` evaluates run_Kf's algebra another way (other association orders,
np.linalg.solve for the 2x2 inverse): the same mathematics, different roundings.  The
distance between the two is the yardstick for the device's own product order.
"""
import math

import numpy as np

import trk_restatement as tr
from trk_restatement import PI, TWO_PI, f32

KF_DEFAULTS = dict(code_disc_sd_chips=0.2, carrier_disc_sd_rads=0.3, code_phase_sd_chips=0.15,
                   carrier_phase_sd_rad=0.25, carrier_freq_sd_hz=0.6, carrier_freq_rate_sd_hz_s=0.01,
                   init_code_phase_sd_chips=0.5, init_carrier_phase_sd_rad=0.7, init_carrier_freq_sd_hz=5.0,
                   init_carrier_freq_rate_sd_hz_s=1.0)  # Kf_Conf::Kf_Conf (kf_conf.cc)


def model(beta, Ti):
    """d_F and d_H of init_kf (:863-869)."""
    TiTi = Ti * Ti
    F = np.array([[1.0, 0.0, beta * Ti, beta * TiTi / 2.0],
                  [0.0, 1.0, 2.0 * PI * Ti, PI * TiTi],
                  [0.0, 0.0, 1.0, Ti],
                  [0.0, 0.0, 0.0, 1.0]])
    H = np.array([[1.0, 0.0, -beta * Ti / 2.0, beta * TiTi / 6.0],
                  [0.0, 1.0, -PI * Ti, PI * TiTi / 3.0]])
    return F, H


def r_of_cn0(cn0_db_hz, Ti, spc):
    """d_R of update_kf_cn0 (:947-954) and update_kf_narrow_integration_time (:921-927)."""
    spc = float(spc)
    lin_ti = math.pow(10.0, cn0_db_hz / 10.0) * Ti
    s2_phase = (1.0 / (2.0 * lin_ti)) * (1.0 + 1.0 / (2.0 * lin_ti))
    s2_tau = (1.0 / lin_ti) * (spc + (spc / (1.0 - spc)) * (1.0 / (2.0 * lin_ti)))
    return np.array([[s2_tau, 0.0], [0.0, s2_phase]])


def hypot_cr(a):
    """float hypot, correctly rounded: exact products, one rounding each in sum, root and cast."""
    x, y = float(a[0]), float(a[1])
    return f32(math.sqrt(x * x + y * y))


def cn0_m2m4(buf, n, coh):
    """cn0_m2m4_estimator (lock_detectors.cc:90-120) as trk_restatement._cn0_m2m4, the two
    log10 correctly rounded."""
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
        return f32(f32(f32(10.0) * f32(np.log10(float(snr)))) - f32(f32(10.0) * f32(np.log10(float(f32(coh))))))


def mm(A, B):
    """A B on lists of Python floats: each element's terms summed in ascending index, every
    product and every sum rounded (no FMA)."""
    return [[sum((A[i][k] * B[k][j] for k in range(1, len(B))), A[i][0] * B[0][j]) for j in range(len(B[0]))]
            for i in range(len(A))]


def _t(A):
    return [list(r) for r in zip(*A)]


def _add(A, B):
    return [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def kf_step(F, H, Q, R, x, P, z, variant="ref"):
    """Prediction and measurement update of run_Kf (:1156-1166): (x_new_new, P_new_new)."""
    if variant == "ref":
        # the reference's expressions, associated left to right as C++ does, every product by
        # mm(): Armadillo's fixed-size code, which a baseline x86-64 build runs without FMA
        # (numpy's BLAS may fuse and reorder, the project's loops keep two roundings per a*b+c)
        F, H, Q, R, P = (np.asarray(a).tolist() for a in (F, H, Q, R, P))
        Ft, Ht = _t(F), _t(H)
        x_no = [r[0] for r in mm(F, [[v] for v in np.asarray(x).tolist()])]
        P_no = _add(mm(mm(F, P), Ft), Q)
        S = _add(mm(mm(H, P_no), Ht), R)
        det = S[0][0] * S[1][1] - S[0][1] * S[1][0]
        Sinv = [[S[1][1] / det, -S[0][1] / det], [-S[1][0] / det, S[0][0] / det]]
        K = mm(mm(P_no, Ht), Sinv)
        Kz = mm(K, [[float(z[0])], [float(z[1])]])
        KH = mm(K, H)
        G = [[(1.0 if i == k else 0.0) - KH[i][k] for k in range(4)] for i in range(4)]
        return np.array([x_no[i] + Kz[i][0] for i in range(4)]), np.array(mm(G, P_no))
    x_no = F @ x
    P_no = F @ (P @ F.T) + Q
    PHt = P_no @ H.T
    S = H @ PHt + R
    K = np.linalg.solve(S.T, PHt.T).T
    return x_no + K @ z, P_no - K @ (H @ P_no)


class KfChannel(tr.Channel):
    """One kf_tracking channel; conf as for Channel, kf: the Kalman values (KF_DEFAULTS)."""

    def __init__(self, conf, kf=None, secondary_code=None, variant="ref"):
        super().__init__(conf, secondary_code)
        self.kf = dict(KF_DEFAULTS)
        if kf is not None:
            self.kf.update({k: float(np.asarray(kf[k]).reshape(-1)[0]) for k in KF_DEFAULTS})
        self.variant = variant
        self.beta = self.chip_rate / self.carrier_hz  # :448

    def start(self, code, acq_delay_samples, acq_doppler_hz, acq_samplestamp, nitems_read, prn=1, data_code=None):
        errs = self.errs  # members that no start_tracking resets
        first = super().start(code, acq_delay_samples, acq_doppler_hz, acq_samplestamp, nitems_read, prn, data_code)
        self.errs = errs
        k = self.kf  # init_kf(0.0, d_carrier_doppler_kf_hz) (:1824)
        self.F, self.H = model(self.beta, self.corr_time)
        self.R = np.diag([math.pow(k["code_disc_sd_chips"], 2.0), math.pow(k["carrier_disc_sd_rads"], 2.0)])
        self.Q = np.diag([math.pow(k[n], 2.0) for n in ("code_phase_sd_chips", "carrier_phase_sd_rad",
                                                        "carrier_freq_sd_hz", "carrier_freq_rate_sd_hz_s")])
        self.Pk = np.diag([math.pow(k[n], 2.0) for n in ("init_code_phase_sd_chips", "init_carrier_phase_sd_rad",
                                                         "init_carrier_freq_sd_hz", "init_carrier_freq_rate_sd_hz_s")])
        self.xk = np.array([0.0, 0.0, float(acq_doppler_hz), 0.0])
        return first

    def _clear_tracking_vars(self):  # :1217-1233
        errs = self.errs
        super()._clear_tracking_vars()
        self.errs = errs

    def _cn0_and_lock(self, coh):  # :1036-1093: the DLL/PLL block's without the EVM
        n = self.p["cn0_samples"]
        if self.cn0_counter < n:
            self.prompt_buffer[self.cn0_counter] = list(self.P)
            self.cn0_counter += 1
            return True
        self.prompt_buffer[self.cn0_counter % n] = list(self.P)
        self.cn0_counter += 1
        self.cn0 = float(self.cn0_smoother.smooth(cn0_m2m4(self.prompt_buffer, n, coh)))
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
        return True

    def _set_shifts(self, narrow):
        if narrow:  # update_kf_narrow_integration_time() before the narrow taps and spc (:1943-1962)
            self._update_kf_narrow()
        super()._set_shifts(narrow)

    def _update_kf_narrow(self):  # :898-935
        Qnew = np.zeros((4, 4))
        F = self.F.tolist()
        for _ in range(self.extend):
            FQFt = np.array(mm(mm(F, np.asarray(self.Q).tolist()), _t(F)))
            Qnew += FQFt
            self.Q = FQFt
        self.Q = Qnew
        self.F, self.H = model(self.beta, self.corr_time)
        self.R = r_of_cn0(self.cn0, self.corr_time, self.spc)

    def _discriminators(self):  # :1131-1151
        if self.cloop:
            with np.errstate(all="ignore"):
                ph = float(f32(math.atan(float(f32(self.P[1] / self.P[0]))))) if self.P[0] != 0 else 0.0
        else:
            ph = float(f32(math.atan2(float(self.P[1]), float(self.P[0]))))
        ph /= TWO_PI
        if self.veml:
            early = math.sqrt(float(f32(f32(f32(f32(self.VE[0] * self.VE[0]) + f32(self.VE[1] * self.VE[1])) +
                                            f32(self.E[0] * self.E[0])) + f32(self.E[1] * self.E[1]))))
            late = math.sqrt(float(f32(f32(f32(f32(self.L[0] * self.L[0]) + f32(self.L[1] * self.L[1])) +
                                           f32(self.VL[0] * self.VL[0])) + f32(self.VL[1] * self.VL[1]))))
            code_err = 0.0 if early + late == 0.0 else (early - late) / (early + late)
        else:
            pe, pl = float(hypot_cr(self.E)), float(hypot_cr(self.L))
            slope = y = f32(1.0)
            code_err = 0.0 if pe + pl == 0.0 else float(f32(f32(y - f32(slope * self.spc)) / slope)) * (pe - pl) / (pe + pl)
        return ph, code_err

    def _run_dll_pll(self):  # run_Kf (:1129-1204); in state 4 after update_kf_cn0 (:2025)
        if self.state == 4:
            _, self.H = model(self.beta, self.corr_time)
            self.R = r_of_cn0(self.cn0, self.corr_time, self.spc)
        ph, code_err = self._discriminators()
        z = np.array([code_err, ph * TWO_PI])
        x, self.Pk = kf_step(self.F, self.H, self.Q, self.R, self.xk, self.Pk, z, self.variant)
        code_error_kf = float(x[0])
        x[0] = 0.0
        self.xk = x
        self.carrier_doppler = float(x[2])
        self.P_old = list(self.P)
        self.code_freq = self.chip_rate + self.carrier_doppler * self.chip_rate / self.carrier_hz
        self.rem_code_samples += self.fs * code_error_kf / self.code_freq
        self.rem_carr = f32(x[1])
        self.errs = [ph, float(f32(x[2])), code_err, code_error_kf]

    def _update_tracking_vars(self):  # :1237-1313
        T_prn_samples = (1.0 / self.code_freq) * float(self.length) * self.fs
        K_blk = T_prn_samples + self.rem_code_samples
        self.current_prn_length_samples = int(math.floor(K_blk))
        self.carrier_phase_step = TWO_PI * self.carrier_doppler / self.fs
        n = float(self.current_prn_length_samples)
        remnant = f32(self.carrier_phase_step * n + 0.5 * self.carrier_phase_rate_step * n * n)
        self.rem_carr = f32(self.rem_carr + remnant)
        self.rem_carr = f32(math.fmod(float(self.rem_carr), TWO_PI))
        self.acc_carrier_phase -= float(remnant)
        self.code_phase_step = self.code_freq / self.fs
        self.rem_code_samples = K_blk - n
        self.rem_code_chips = self.code_freq * self.rem_code_samples / self.fs

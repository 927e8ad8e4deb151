"""Oracle comparisons shared by the acquisition GPU tests (not a test module).

Tolerances (BASELINE.json north_star): CAF peak, input power, second peak and test
statistic within 1e-4 relative (fp32); Doppler index and code phase equal, or -- the
near-tie rule of SURVEY §7 H3 -- the oracle's grid value at the GPU's cell within
1e-4 of the oracle's maximum.
"""
import json
import os

import numpy as np

import gsdr
from gsdr import synth
from oracle import pcps

RTOL = 1e-4
SPECTRUM_TOL = 2e-6  # norm-relative error of the forward spectra (test_large_fft_four_step)
GRID_TOL = 1e-5      # max |g - M| over M.max() of a dumped |R|^2 grid


def _codes(prns, fs, n):
    return np.stack([synth.gps_ca_sampled(p, fs, n) for p in prns])


def _oracle_grids(x, codes, fs, dmax, dstep, D):
    N = len(x)
    wipe = pcps.doppler_wipeoffs(fs, N, dmax, dstep, D)
    grids = []
    for c in codes:
        cf = pcps.fft_code(c, N, N)
        grids.append(pcps.magnitude_grid(x, wipe, cf))
    return grids


def _check_result(r, M, pfa, spc, fs, dmax, dstep, spcode):
    """Compare one GPU result record with the oracle statistics of grid M."""
    N = M.shape[1]
    if pfa > 0:
        ti, di, gmax, ip, stat = pcps.max_to_input_power_statistic(M)
    else:
        ti, di, gmax, second, stat = pcps.first_vs_second_peak_statistic(M, spc, N)
    same_cell = (r["doppler_index"] == di and r["code_phase"] == ti)
    if not same_cell:  # near tie (H3)
        assert abs(M[r["doppler_index"], r["code_phase"]] - gmax) <= RTOL * gmax, (r, ti, di)
        return False
    assert abs(r["peak"] - gmax) <= RTOL * gmax
    assert r["doppler_hz"] == pcps.doppler_hz(di, dmax, dstep)
    assert r["acq_delay_samples"] == float(np.fmod(np.float32(ti), np.float32(spcode)))
    if pfa > 0:
        assert abs(r["input_power"] - ip) <= RTOL * ip
    else:
        assert abs(r["second_peak"] - second) <= RTOL * second
    assert abs(r["test_statistic"] - stat) <= RTOL * stat
    return True


def _oracle_attempt(chunks, codes, pfa, D, dmax, dstep, bit_transition, spc, threshold, fs=4000000):
    """Per PRN: (dwell index, ti, di, peak, input_power/second, stat) of the decision."""
    N = len(chunks[0])
    wipe = pcps.doppler_wipeoffs(fs, N, dmax, dstep, D)
    out = []
    for code in codes:
        cf = pcps.fft_code(code, N, N, bit_transition=bit_transition)
        acc = None
        for k, x in enumerate(chunks):
            M = pcps.magnitude_grid(x, wipe, cf, bit_transition=bit_transition)
            acc = M if acc is None else (acc + M).astype(np.float32)
            if pfa > 0:
                ti, di, peak, ip, stat = pcps.max_to_input_power_statistic(acc, k + 1)
                aux = ip
            else:
                full = np.zeros((D, N), np.float32)
                full[:, :acc.shape[1]] = acc
                ti, di, peak, aux, stat = pcps.first_vs_second_peak_statistic(full, spc, N)
            if stat > threshold or k + 1 == len(chunks):
                out.append((k, ti, di, peak, aux, stat, acc))
                break
    return out


def _check(r, o, pfa):
    """Compare one GPU record of a dwell / bit-transition attempt with _oracle_attempt's."""
    k, ti, di, peak, aux, stat, acc = o
    assert r["num_dwells"] == k + 1
    if (r["doppler_index"], r["code_phase"]) != (di, ti):  # near tie
        assert abs(acc[r["doppler_index"], r["code_phase"]] - peak) <= RTOL * peak
        return
    assert abs(r["peak"] - peak) <= RTOL * peak
    assert abs(r["test_statistic"] - stat) <= RTOL * stat
    if pfa > 0:
        assert abs(r["input_power"] - aux) <= RTOL * aux
    else:
        assert abs(r["second_peak"] - aux) <= RTOL * aux


# ---------------------------------------------------------------- one-block size cases
# One block of 1 ms GPS C/A at fs = 1000 N (FFT size N), 4 PRN slots: three visible at
# 50 dB-Hz inside the +-1000 Hz / 250 Hz grid (8 Doppler rows) and one absent.
SWEEP_DMAX, SWEEP_DSTEP = 1000, 250
PEAK_RATIO_THRESHOLD = 2.5  # set_threshold for the pfa = 0 handles


class SizeCase:
    """The input and the fp64 oracle of one FFT size, computed once (size_case)."""

    def __init__(self, N, dmax=SWEEP_DMAX, dstep=SWEEP_DSTEP):
        self.N, self.fs, self.dmax, self.dstep = N, 1000 * N, dmax, dstep
        self.D = pcps.num_doppler_bins(dmax, dstep)
        self.sats = synth.random_constellation(3, seed_offset=N, cn0_dbhz=50.0, max_doppler=dmax - 100.0)
        self.x = synth.gps_l1_iq(self.fs, N, self.sats, seed_offset=N)
        vis = [s.prn for s in self.sats]
        absent = next(p for p in range(1, 33) if p not in vis)
        self.prns = np.array(vis + [absent])
        self.nvis = len(vis)
        self.codes = _codes(self.prns, self.fs, N)
        self.spc = int(np.ceil(self.fs / 1023000.0))
        self.spcode = float(np.float32(self.fs) * np.float32(0.001))
        wipe = pcps.doppler_wipeoffs(self.fs, N, dmax, dstep, self.D)
        self.spectra = np.fft.fft(self.x.astype(np.complex128)[None, :] * wipe.astype(np.complex128), axis=1)
        self.grids = list(pcps.magnitude_grids(self.x, wipe, [pcps.fft_code(c, N, N) for c in self.codes]))
        for a in [self.x, self.codes, self.spectra] + self.grids:
            a.setflags(write=False)


_size_cases = {}


def size_case(N, dmax=SWEEP_DMAX, dstep=SWEEP_DSTEP):
    """SizeCase(N), kept for the cases of the same size that follow (the last two sizes)."""
    key = (N, dmax, dstep)
    if key not in _size_cases:
        while len(_size_cases) >= 2:
            _size_cases.pop(next(iter(_size_cases)))
        _size_cases[key] = SizeCase(N, dmax, dstep)
    return _size_cases[key]


def make_acq(case, pfa, nprn=None, **kw):
    """A handle for `case` with its first nprn codes set and, in peak-ratio mode, the threshold."""
    nprn = len(case.prns) if nprn is None else nprn
    acq = gsdr.Acquisition(case.fs, case.N, case.dmax, case.dstep, pfa=pfa, max_prns=len(case.prns), **kw)
    assert acq.fft_size == case.N and acq.num_doppler_bins == case.D
    acq.set_local_codes(case.codes[:nprn], case.prns[:nprn])
    if not pfa > 0:
        acq.set_threshold(PEAK_RATIO_THRESHOLD)
    return acq


def spectrum_error(acq, case):
    """Norm-relative error of the dumped forward spectra against fp64, over every Doppler row."""
    X = acq.dump_spectra(case.x)
    return float(np.abs(X - case.spectra).max() / np.abs(case.spectra).max())


def grid_error(acq, case, slot=0):
    """max |g - M| / M.max() of the dumped |R|^2 grid of a PRN slot against the oracle grid."""
    g = acq.dump_grid(case.x, slot)
    M = case.grids[slot]
    return float(np.max(np.abs(g.astype(np.float64) - M)) / M.max())


def check_records(res, acq, case, pfa):
    """The result records of one block against the oracle: every visible PRN on the
    oracle's cell, at most one of the slots on the near-tie branch, `positive` equal
    wherever the oracle statistic is further than 1e-3 relative from the threshold."""
    thr = acq.threshold
    if pfa > 0:
        ref = pcps.threshold(pfa, case.N, case.D)
        assert abs(thr - ref) <= 1e-6 * ref
    exact = []
    for p in range(len(res)):
        assert res[p]["prn"] == case.prns[p]
        exact.append(_check_result(res[p], case.grids[p], pfa, case.spc, case.fs, case.dmax, case.dstep, case.spcode))
        if pfa > 0:
            stat = pcps.max_to_input_power_statistic(case.grids[p])[4]
        else:
            stat = pcps.first_vs_second_peak_statistic(case.grids[p], case.spc, case.N)[4]
        if abs(stat - thr) > 1e-3 * thr:
            assert bool(res[p]["positive"]) == bool(stat > thr), (p, stat, thr)
    assert all(exact[:case.nvis]), exact
    assert sum(exact) >= len(res) - 1, exact
    return exact


def check_size(acq, case, pfa, tag):
    """The three checks of one handle: forward spectra, the grid of a visible PRN and the
    result records; the measured errors are printed (and logged to GSDR_PARITY_LOG)
    before they are asserted."""
    plan = acq.plan
    es = spectrum_error(acq, case)
    eg = grid_error(acq, case, 0)
    line = {"tag": tag, "N": case.N, "pfa": pfa, "plan": plan, "spectrum_err": es, "grid_err": eg}
    print("parity acq", json.dumps(line))
    if os.environ.get("GSDR_PARITY_LOG"):
        with open(os.environ["GSDR_PARITY_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")
    assert es < SPECTRUM_TOL, line
    assert eg <= GRID_TOL, line
    res = acq.run(case.x)[0]
    check_records(res, acq, case, pfa)
    return res

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


def _oracle_grids(x, codes, fs, dmax, dstep, D, doppler_center=0, doppler_bias=0, mode="exact"):
    N = len(x)
    wipe = pcps.doppler_wipeoffs(fs, N, dmax, dstep, D, doppler_center, doppler_bias, mode)
    grids = []
    for c in codes:
        cf = pcps.fft_code(c, N, N)
        grids.append(pcps.magnitude_grid(x, wipe, cf))
    return grids


def _check_result(r, M, pfa, spc, fs, dmax, dstep, spcode, doppler_center=0, doppler_bias=0, mode="exact"):
    """Compare one GPU result record with the oracle statistics of grid M (built with the
    same centre, bias and carrier model).  The reported Doppler carries the centre and not
    the bias (pcps_acquisition.cc:302-303 against :535)."""
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
    assert r["doppler_hz"] == pcps.doppler_hz(di, dmax, dstep, doppler_center)
    assert r["acq_delay_samples"] == float(np.fmod(np.float32(ti), np.float32(spcode)))
    if pfa > 0:
        assert abs(r["input_power"] - ip) <= RTOL * ip
    else:
        assert abs(r["second_peak"] - second) <= RTOL * second
    assert abs(r["test_statistic"] - stat) <= RTOL * stat
    return True


def _oracle_attempt(chunks, codes, pfa, D, dmax, dstep, bit_transition, spc, threshold, fs=4000000,
                    doppler_center=0, doppler_bias=0, mode="exact"):
    """Per PRN: (dwell index, ti, di, peak, input_power/second, stat) of the decision."""
    N = len(chunks[0])
    wipe = pcps.doppler_wipeoffs(fs, N, dmax, dstep, D, doppler_center, doppler_bias, mode)
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


# ---------------------------------------------------------------- the per-call dwell
def oracle_dwell_sequence(chunks, codes, pfa, D, dmax, dstep, bit_transition, spc, fs=4000000, doppler_center=0,
                          doppler_bias=0, mode="exact"):
    """acquisition_core called once per block (gsdr_acq_run_dwell): per PRN and dwell k the
    (ti, di, peak, input_power | second_peak, stat, acc_grid) of the grid accumulated over
    chunks 0..k -- a float32 add per dwell, the CFAR divisor k + 1, the peak-ratio window
    wrapping at fft_size.  Every dwell is reported: the caller's FSM decides when to stop."""
    N = len(chunks[0])
    wipe = pcps.doppler_wipeoffs(fs, N, dmax, dstep, D, doppler_center, doppler_bias, mode)
    out = []
    for code in codes:
        cf = pcps.fft_code(code, N, N, bit_transition=bit_transition)
        acc, seq = None, []
        for k, x in enumerate(chunks):
            M = pcps.magnitude_grid(x, wipe, cf, bit_transition=bit_transition)
            acc = M if acc is None else (acc + M).astype(np.float32)
            if pfa > 0:
                ti, di, peak, aux, stat = pcps.max_to_input_power_statistic(acc, k + 1)
            else:
                full = np.zeros((D, N), np.float32)
                full[:, :acc.shape[1]] = acc
                ti, di, peak, aux, stat = pcps.first_vs_second_peak_statistic(full, spc, N)
            acc.setflags(write=False)
            seq.append((ti, di, peak, aux, stat, acc))
        out.append(seq)
    return out


def check_dwell_record(r, o, pfa, k, stamp, thr, dmax, dstep, spcode, doppler_center=0):
    """One record of run_dwell(x_k, k, stamp) against oracle_dwell_sequence's entry o of
    that PRN and dwell, by the rules of _check / _check_result / check_records.  Returns
    whether the record is on the oracle's cell (False: the near-tie branch)."""
    ti, di, peak, aux, stat, acc = o
    assert r["num_dwells"] == k + 1
    assert r["samplestamp"] == stamp
    assert r["doppler_hz"] == pcps.doppler_hz(int(r["doppler_index"]), dmax, dstep, doppler_center)
    assert r["acq_delay_samples"] == float(np.fmod(np.float32(r["code_phase"]), np.float32(spcode)))
    if (r["doppler_index"], r["code_phase"]) != (di, ti):  # near tie
        assert abs(acc[r["doppler_index"], r["code_phase"]] - peak) <= RTOL * peak, (r, ti, di)
        return False
    assert abs(r["peak"] - peak) <= RTOL * peak
    assert abs(r["test_statistic"] - stat) <= RTOL * stat
    if pfa > 0:
        assert abs(r["input_power"] - aux) <= RTOL * aux
    else:
        assert abs(r["second_peak"] - aux) <= RTOL * aux
    if abs(stat - thr) > 1e-3 * thr:
        assert bool(r["positive"]) == bool(stat > thr), (r, stat, thr)
    return True


def row_maxima_margin(acc):
    """(largest - second largest) / largest of the row maxima of an accumulated grid: the
    distance of the oracle's Doppler row from a near tie."""
    m = np.sort(acc.max(axis=1).astype(np.float64))
    return float((m[-1] - m[-2]) / m[-1])


DWELL_MARGIN = 1e-3  # every visible PRN's row_maxima_margin, at every dwell, exceeds this


class DwellCase:
    """K blocks of one signal at FFT size N, 4 PRN slots (three visible, then one absent)
    on the +-1000 Hz / 250 Hz grid, and the fp64 oracle's dwell sequence of both
    statistics, computed once (dwell_case).  kind: "gps" (1 ms C/A at fs = 1000 N, or
    N / 2 per ms with bit_transition), "gal" (4 ms Galileo E1 at 8 Msps, N = 32000)."""

    def __init__(self, kind, N, K, seed, cn0, bit_transition=False, delays=None, center=0):
        self.kind, self.N, self.K, self.bt, self.center = kind, N, K, bit_transition, center
        self.dmax, self.dstep = SWEEP_DMAX, SWEEP_DSTEP
        self.D = pcps.num_doppler_bins(self.dmax, self.dstep)
        nblocks = 2 * K  # two attempts: chunks 0..K-1 and K..2K-1
        rng = np.random.default_rng(seed)
        if kind == "gal":
            self.fs, vis = 8000000, [4, 19, 27]
            sats = [synth.GalileoSatellite(p, center + float(rng.uniform(-900, 900)), float(rng.uniform(0, 4092)),
                                           cn0, float(rng.uniform(0, 6.28))) for p in vis]
            self.x = synth.gal_e1_iq(self.fs, nblocks * N, sats, seed_offset=seed)
            self.prns = np.array(vis + [7])
            self.codes = np.stack([synth.gal_e1_sampled(int(p), self.fs) for p in self.prns])
            self.kw = dict(sampled_ms=4, ms_per_code=4, samples_per_code=float(N))
            self.spcode = float(N)
        else:
            self.fs = 1000 * (N // 2 if bit_transition else N)
            sats = synth.random_constellation(3, seed_offset=seed, cn0_dbhz=cn0, max_doppler=900.0)
            for i, s in enumerate(sats):
                s.doppler_hz += center
                if delays is not None and delays[i] is not None:
                    s.code_delay_chips = delays[i]
            self.x = synth.gps_l1_iq(self.fs, nblocks * N, sats, seed_offset=seed)
            vis = [s.prn for s in sats]
            self.prns = np.array(vis + [next(p for p in range(1, 33) if p not in vis)])
            self.codes = np.stack([np.resize(synth.gps_ca_sampled(int(p), self.fs), N) for p in self.prns])
            self.kw = {}
            self.spcode = float(np.float32(self.fs) * np.float32(0.001))
        self.nvis = 3
        self.spc = int(np.ceil(self.fs / 1023000.0))
        self.chunks = [self.x[k * N:(k + 1) * N] for k in range(nblocks)]
        self._seq = {}
        for a in (self.x, self.codes):
            a.setflags(write=False)

    def seq(self, pfa, first=0):
        """oracle_dwell_sequence of chunks first .. first + K - 1."""
        key = (pfa > 0, first)
        if key not in self._seq:
            self._seq[key] = oracle_dwell_sequence(self.chunks[first:first + self.K], self.codes, pfa, self.D,
                                                   self.dmax, self.dstep, self.bt, self.spc, fs=self.fs,
                                                   doppler_center=self.center)
        return self._seq[key]

    def threshold(self, pfa, max_dwells=None):
        K = self.K if max_dwells is None else max_dwells
        return pcps.threshold(pfa, self.N, self.D, K, self.bt) if pfa > 0 else PEAK_RATIO_THRESHOLD

    def make(self, pfa, nprn=None, max_dwells=None, center=None, **kw):
        """A handle with max_prns above the active count, the first nprn codes set."""
        nprn = len(self.prns) if nprn is None else nprn
        K = self.K if max_dwells is None else max_dwells
        kw = dict(self.kw, **kw)
        acq = gsdr.Acquisition(self.fs, self.N, self.dmax, self.dstep, pfa=pfa, max_prns=len(self.prns) + 2,
                               max_dwells=K, bit_transition=self.bt,
                               doppler_center=self.center if center is None else center, **kw)
        assert acq.fft_size == self.N and acq.num_doppler_bins == self.D
        acq.set_local_codes(self.codes[:nprn], self.prns[:nprn])
        thr = self.threshold(pfa, K)
        if pfa > 0:
            assert abs(acq.threshold - thr) <= 1e-6 * thr
        else:
            acq.set_threshold(thr)
        return acq

    def check(self, recs, pfa, k, stamp, first=0, max_dwells=None):
        """The records of run_dwell(chunks[first + k], k, stamp): every visible PRN on the
        oracle's cell, at most the absent one on the near-tie branch."""
        seq = self.seq(pfa, first)
        thr = self.threshold(pfa, max_dwells)
        exact = []
        for p in range(len(recs)):
            assert recs[p]["prn"] == self.prns[p]
            exact.append(check_dwell_record(recs[p], seq[p][k], pfa, k, stamp, thr, self.dmax, self.dstep,
                                            self.spcode, self.center))
        assert all(exact[:self.nvis]), exact
        return exact


# (kind, N, K, seed, cn0, bit_transition, delays): the inputs of test_gpu_acq_dwell_calls.py
# and test_gpu_acq_doppler_grid.py; test_oracle_acq_grid.py pins their near-tie margins.
DWELL_CASES = {
    "lds4000": ("gps", 4000, 3, 401, 48.0, False, None),
    "runtime6000": ("gps", 6000, 3, 402, 48.0, False, None),
    "four40000": ("gps", 40000, 3, 403, 48.0, False, None),
    "packed32000": ("gal", 32000, 2, 404, 46.0, False, None),
    "split25000": ("gps", 25000, 1, 405, 48.0, False, None),
    # bit transition: satellite 0 within samples_per_chip of the start of the half row,
    # satellite 1 within samples_per_chip of its end (BT_DELAYS, in chips)
    "bt8000": ("gps", 8000, 1, 406, 50.0, True, (0.3, 1022.3, None)),
    "bt12000": ("gps", 12000, 1, 407, 50.0, True, (0.3, 1022.3, None)),
    # the per-call dwell on a grid moved by set_doppler (centre 500), two attempts
    "moved4000": ("gps", 4000, 2, 410, 48.0, False, None),
}
DWELL_CASE_CENTER = {"moved4000": 500}
_dwell_cases = {}


def dwell_case(name):
    if name not in _dwell_cases:
        kind, N, K, seed, cn0, bt, delays = DWELL_CASES[name]
        _dwell_cases[name] = DwellCase(kind, N, K, seed, cn0, bt, delays, DWELL_CASE_CENTER.get(name, 0))
    return _dwell_cases[name]


# ---------------------------------------------------------------- one-block size cases
# One block of 1 ms GPS C/A at fs = 1000 N (FFT size N), 4 PRN slots: three visible at
# 50 dB-Hz inside the +-1000 Hz / 250 Hz grid (8 Doppler rows) and one absent.
SWEEP_DMAX, SWEEP_DSTEP = 1000, 250
PEAK_RATIO_THRESHOLD = 2.5  # set_threshold for the pfa = 0 handles


class SizeCase:
    """The input and the fp64 oracle of one FFT size, computed once (size_case).  center,
    bias and mode move the Doppler grid (doppler_center), offset the carriers
    (doppler_bias) and pick the oracle's carrier model: the satellites' Dopplers move with
    the centre, and the block is multiplied by exp(+2 pi j bias n / fs) in float64 before
    its one rounding to complex64, so that the biased grid finds them."""

    def __init__(self, N, dmax=SWEEP_DMAX, dstep=SWEEP_DSTEP, center=0, bias=0, mode="exact", seed=None):
        seed = N if seed is None else seed
        self.N, self.fs, self.dmax, self.dstep = N, 1000 * N, dmax, dstep
        self.center, self.bias, self.mode = center, bias, mode
        self.D = pcps.num_doppler_bins(dmax, dstep)
        self.sats = synth.random_constellation(3, seed_offset=seed, cn0_dbhz=50.0, max_doppler=dmax - 100.0)
        for s in self.sats:
            s.doppler_hz += center
        if bias:
            x = synth.gps_l1_iq(self.fs, N, self.sats, seed_offset=seed, dtype=np.complex128)
            t = float(bias) * np.arange(N, dtype=np.float64) / float(self.fs)
            self.x = (x * np.exp(2j * np.pi * (t - np.floor(t)))).astype(np.complex64)
        else:
            self.x = synth.gps_l1_iq(self.fs, N, self.sats, seed_offset=seed)
        vis = [s.prn for s in self.sats]
        absent = next(p for p in range(1, 33) if p not in vis)
        self.prns = np.array(vis + [absent])
        self.nvis = len(vis)
        self.codes = _codes(self.prns, self.fs, N)
        self.spc = int(np.ceil(self.fs / 1023000.0))
        self.spcode = float(np.float32(self.fs) * np.float32(0.001))
        wipe = pcps.doppler_wipeoffs(self.fs, N, dmax, dstep, self.D, center, bias, mode)
        self.spectra = np.fft.fft(self.x.astype(np.complex128)[None, :] * wipe.astype(np.complex128), axis=1)
        self.grids = list(pcps.magnitude_grids(self.x, wipe, [pcps.fft_code(c, N, N) for c in self.codes]))
        for a in [self.x, self.codes, self.spectra] + self.grids:
            a.setflags(write=False)


_size_cases = {}


def size_case(N, dmax=SWEEP_DMAX, dstep=SWEEP_DSTEP, center=0, bias=0, mode="exact", seed=None):
    """SizeCase(N), kept for the cases of the same size that follow (the last two sizes)."""
    key = (N, dmax, dstep, center, bias, mode, seed)
    if key not in _size_cases:
        while len(_size_cases) >= 2:
            _size_cases.pop(next(iter(_size_cases)))
        _size_cases[key] = SizeCase(N, dmax, dstep, center, bias, mode, seed)
    return _size_cases[key]


def make_acq(case, pfa, nprn=None, **kw):
    """A handle for `case` with its first nprn codes set and, in peak-ratio mode, the threshold."""
    nprn = len(case.prns) if nprn is None else nprn
    kw.setdefault("doppler_center", case.center)
    kw.setdefault("doppler_bias", case.bias)
    acq = gsdr.Acquisition(case.fs, case.N, case.dmax, case.dstep, pfa=pfa, max_prns=len(case.prns), **kw)
    assert acq.fft_size == case.N and acq.num_doppler_bins == case.D
    if case.mode != "exact":
        acq.set_wipeoff(case.mode)
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
        exact.append(_check_result(res[p], case.grids[p], pfa, case.spc, case.fs, case.dmax, case.dstep, case.spcode,
                                   case.center, case.bias, case.mode))
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


# ---------------------------------------------------------------- moved / biased Doppler grids
# One N = 4000 block at 4 Msps on three forward-spectrum layouts (gsdr_acq_get_spectrum_reuse):
# 250 Hz steps of the 1 kHz bins share q = 4 spectra (shift p = 1); the replayed generic
# protokernel is not shift-invariant and 300 Hz steps (p / q = 3 / 10, q > D / 2) do not
# pay, so both keep one spectrum per row.
GRID_N, GRID_SEED = 4000, 422
GRID_LAYOUTS = {  # name: (doppler_max, doppler_step, carrier model, spectrum_reuse)
    "reuse": (1000, 250, "exact", (4, 1)),
    "generic": (1000, 250, "generic", (8, 0)),
    "step300": (1200, 300, "exact", (8, 0)),
}
GRID_CENTERS = (500, -375, 2500)  # a multiple of the step, none, every row above zero
GRID_BIASES = ((562500, 0), (562500, 500), (-1687500, 0), (-1687500, 500))  # GLONASS L1 k = +1, -3; centre


def grid_args(layout, center, bias=0):
    """size_case's arguments of a layout with the grid moved / biased."""
    dmax, dstep, mode, _ = GRID_LAYOUTS[layout]
    return (GRID_N, dmax, dstep, center, bias, mode, GRID_SEED)


GRID_CASES = {name: [grid_args(name, c) for c in GRID_CENTERS] + [grid_args(name, c, b) for b, c in GRID_BIASES]
              for name in GRID_LAYOUTS}

# gsdr_acq_set_doppler on a live handle: (doppler_max, doppler_step, doppler_center) after
# each call, from a handle created at (1000, 250, 0) -- the centre alone, the step with
# the 8 rows kept (reuse q = 4 -> 2), the plain layout, and back; per FFT size (25000: the
# split correlate, the centre and one step change).
SET_DOPPLER_CHAIN = ((1000, 250, 500), (1000, 250, -375), (2000, 500, -375), (1200, 300, -375), (1000, 250, 0))
SET_DOPPLER_SIZES = {4000: SET_DOPPLER_CHAIN, 6000: SET_DOPPLER_CHAIN, 25000: ((1000, 250, 500), (2000, 500, 500))}


def chain_args(N, step):
    """size_case's arguments of one step of the chain: the satellites inside that grid."""
    dmax, dstep, center = step
    return (N, dmax, dstep, center, 0, "exact", GRID_SEED)

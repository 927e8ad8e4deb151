"""Float64 restatement of the QuickSync acquisition block and the inputs its tests share.

Written from the reference's text, not from the engine's formulation:
  pcps_quicksync_acquisition_cc.cc
    :64, :87   an item is sampled_ms * samples_per_ms = p spc samples; d_fft_size = spc / p = Nf;
    :135-157   set_local_code: the code kept unfolded; conj(FFT) of the sum of its p segments;
    :286       fft_normalization_factor = float(Nf) float(Nf);
    :288-293   d_input_power, d_mag, d_test_statistics zeroed in every state-1 call; the sample
               counter advanced by the item before the grid;
    :310-312   d_input_power = sum |x|^2 / L;
    :329-343   per Doppler row: the item times the row's wipe-off (L samples), folded into Nf
               points as the sum of its p^2 segments;
    :347-367   FFT, times the code spectrum, inverse FFT, |.|^2, index_max (first maximum),
               magt = max / (norm norm);
    :370       if d_mag < magt: the row takes over;
    :383-418   the p delays indext + i Nf: acc_i = sum_j t[delay_i + j] code[j] (no conjugate),
               index_max of |acc_i|^2 names the delay; Acq_delay_samples, Acq_doppler_hz,
               Acq_samplestamp_samples = d_sample_counter (the end of the item), Acq_doppler_step;
    :421       d_test_statistics = d_mag / d_input_power;
    :443-467   the decision, without and with bit transition;
    :239-548   the state machine (0 stand-by, 1 one item per call, 2 / 3 publish 1 / 2).
  gps_l1_ca_pcps_quicksync_acquisition.cc
    :264-281   calculate_threshold.
The Doppler wipe-off is the exact carrier exp(-j 2 pi f n / fs) (the engine's default model).
"""
import functools

import numpy as np

from gsdr import synth

MIN_MARGIN = 1e-3   # every comparison of an index, row or candidate first pins the winner this far above its runner-up
RTOL = 1e-4         # the project's acquisition tolerance
NITEMS = 3


def doppler_rows(dmax, dstep):
    """The bins init() counts (:178-185) and their frequencies (:191, :324)."""
    return [-dmax + dstep * i for i in range(len(range(-dmax, dmax + 1, dstep)))]


def index_max(m):
    """volk_gnsssdr_32f_index_max_32u: the first maximum."""
    return int(np.argmax(m))


def input_power(x):
    x = np.asarray(x, np.complex128)
    return float(np.sum(x.real ** 2 + x.imag ** 2) / len(x))


def wipeoff(f, fs, L):
    n = np.arange(L, dtype=np.float64)
    return np.exp(-2j * np.pi * ((f * n / fs) % 1.0))


def fold(v, nf):
    """The sum of the len(v) / nf segments of v (:146-151, :336-343)."""
    return np.asarray(v, np.complex128).reshape(-1, nf).sum(axis=0)


def _margin(m, i):
    """(winner - runner-up) / winner of the values m whose winner is m[i]."""
    others = np.delete(np.asarray(m, np.float64), i)
    return float((m[i] - others.max()) / m[i]) if len(others) else 1.0


def grid_rows(x, fs, dmax, dstep, code, p):
    """-> mags [D], idx [D], idx_margin [D]: per Doppler row the normalised maximum of the folded
    correlation (magt, :367), its first-maximum index and (best - second best) / best in the row."""
    spc = len(code)
    nf = spc // p
    L = p * spc
    x = np.asarray(x, np.complex128)
    assert len(x) == L and spc % p == 0
    norm = (float(nf) * float(nf)) ** 2
    cf = np.conj(np.fft.fft(fold(code, nf)))
    mags, idx, marg = [], [], []
    for f in doppler_rows(dmax, dstep):
        X = np.fft.fft(fold(x * wipeoff(f, fs, L), nf))
        r = np.fft.ifft(X * cf) * nf  # the unnormalised inverse transform
        m = r.real ** 2 + r.imag ** 2
        i = index_max(m)
        mags.append(m[i] / norm)
        idx.append(i)
        marg.append(_margin(m, i))
    return np.array(mags), np.array(idx), np.array(marg)


def candidates(x, fs, f, code, p, indext):
    """:383-412 -> the p values |acc_i|^2 for the delays indext + i Nf on the row of frequency f."""
    spc = len(code)
    nf = spc // p
    t = np.asarray(x, np.complex128) * wipeoff(f, fs, p * spc)
    c = np.asarray(code, np.complex128)
    out = []
    for i in range(p):
        delay = indext % spc + i * nf
        acc = np.sum(t[delay:delay + spc] * c)
        out.append(acc.real ** 2 + acc.imag ** 2)
    return np.array(out)


def item_record(x, fs, dmax, dstep, code, p, stamp):
    """One item's grid from d_mag = 0: the record gsdr_acq_run_quicksync owes (its samplestamp the
    item's first sample, `stamp`), the rows, the winner's candidate powers and the margins."""
    spc = len(code)
    nf = spc // p
    rows = doppler_rows(dmax, dstep)
    mags, idx, im = grid_rows(x, fs, dmax, dstep, code, p)
    d_mag, d = 0.0, None
    for k in range(len(rows)):
        if d_mag < mags[k]:  # :370
            d_mag, d = mags[k], k
    cand = candidates(x, fs, rows[d], code, p, int(idx[d]))
    i = index_max(cand)
    ip = input_power(x)
    rec = dict(doppler_index=d, folded_phase=int(idx[d]), candidate=i, doppler_hz=rows[d], mag=float(d_mag),
               input_power=ip, test_statistic=float(d_mag) / ip, candidate_power=float(cand[i]),
               acq_delay_samples=float(int(idx[d]) % spc + i * nf), samplestamp=int(stamp))
    margins = dict(row=_margin(mags, d), index=float(im[d]), candidate=_margin(cand, i))
    return dict(rec=rec, mags=mags, idx=idx, cand=cand, margins=margins)


def decide(records, threshold, bit_transition, max_dwells):
    """:443-467 over one satellite's per-item records (dicts of item_record), one per state-1
    call -> (record, positive, num_dwells); positive None if the records end first."""
    for k, r in enumerate(records):
        stat = r["test_statistic"]  # d_test_statistics is this call's alone (:290, :421)
        if not bit_transition:
            if stat > threshold:
                return r, True, k + 1
            if k + 1 == max_dwells:
                return r, False, k + 1
        elif k + 1 == max_dwells:
            return r, stat > threshold, k + 1
    return r, None, len(records)


def threshold(pfa, spc, p, dmax, dstep):
    """calculate_threshold (adapter :264-281): pfa is a float, 1.0 - pfa a double, ncells an
    unsigned product of integer quotients, the quantile -log1p(-val) / lambda, cast to float."""
    ncells = (spc // p) * len(doppler_rows(dmax, dstep))
    val = (1.0 - float(np.float32(pfa))) ** (1.0 / float(ncells))
    lam = float(spc) / float(p)
    return float(np.float32(-np.log1p(-val) / lam))


def default_folding_factor(spc):
    """adapter :70."""
    return int(np.ceil(np.sqrt(np.log2(spc))))


def sampled_ms_key(value, p):
    """coherent_integration_time_ms as the adapter rounds it (adapter :73-89)."""
    if value % p == 0:
        return value
    return p if value < p else (value // p) * p


class RefBlock:
    """general_work (:223-550) over items of L = p spc samples."""

    def __init__(self, fs, spc, p, dmax, dstep, max_dwells, threshold, bit_transition, code, grid=None):
        # grid: item -> the dict of item_record's "rec", for driving the state machine on given outcomes
        self.grid = grid or (lambda item: item_record(item, fs, dmax, dstep, code, p, 0)["rec"])
        self.fs, self.spc, self.p, self.dmax, self.dstep = fs, spc, p, dmax, dstep
        self.L = p * spc
        self.max_dwells, self.threshold, self.bit_transition, self.code = max_dwells, threshold, bit_transition, code
        self.state, self.active, self.sample_counter, self.well_count = 0, False, 0, 0
        self.mag = self.ip = self.stat = 0.0
        self.synchro = dict(acq_delay_samples=0.0, acq_doppler_hz=0.0, acq_samplestamp_samples=0, acq_doppler_step=0)

    def _restart(self):
        self.synchro = dict(acq_delay_samples=0.0, acq_doppler_hz=0.0, acq_samplestamp_samples=0, acq_doppler_step=0)
        self.well_count, self.mag, self.ip, self.stat = 0, 0.0, 0.0, 0.0

    def work(self, items):
        """items: the ninput_items items offered -> (consumed, event)."""
        n = len(items)
        if self.state == 0:
            if self.active:
                self._restart()
                self.state = 1
            self.sample_counter += self.L * n
            return n, 0
        if self.state == 1:
            self.ip = self.mag = self.stat = 0.0  # :288-290
            self.sample_counter += self.L         # :293
            self.well_count += 1
            b = self.grid(items[0])
            self.ip = b["input_power"]
            if self.mag < b["mag"]:  # true for every finite positive grid; :381 is then true as well
                self.mag = b["mag"]
                self.synchro = dict(acq_delay_samples=b["acq_delay_samples"], acq_doppler_hz=float(b["doppler_hz"]),
                                    acq_samplestamp_samples=self.sample_counter, acq_doppler_step=self.dstep)
                self.stat = self.mag / self.ip
            if not self.bit_transition:
                if self.stat > self.threshold:
                    self.state = 2
                elif self.well_count == self.max_dwells:
                    self.state = 3
            elif self.well_count == self.max_dwells:
                self.state = 2 if self.stat > self.threshold else 3
            return 1, 0
        event = 1 if self.state == 2 else 2
        self.active = False
        self.state = 0
        self.sample_counter += self.L * n
        return n, event


def run_attempts(block, x, attempts, per_call=1):
    """The self-test driver's loop (host/tests/quicksync_acquisition_selftest.cc) on a RefBlock."""
    L, offset, out = block.L, 0, []
    for _ in range(attempts):
        block.active = True
        calls, event = [], 0
        while event == 0 and offset + L <= len(x):
            offered = min(per_call, (len(x) - offset) // L)
            state = block.state
            c, event = block.work([x[offset + i * L:offset + (i + 1) * L] for i in range(offered)])
            offset += c * L
            calls.append(dict(state=state, offered=offered, consumed=c, event=event, mag=block.mag,
                              input_power=block.ip, test_statistic=block.stat, **block.synchro))
        out.append(dict(calls=calls, event=event, end_state=block.state, sample_counter=block.sample_counter))
    return out


# ---------------------------------------------------------------- the shared cases
#   case       fs       spc    p  Nf    L       D  reaches
#   q4000x2    4 Msps   4000   2  2000  8000    9  compile-time plan
#   q4000x4    4 Msps   4000   4  1000  16000   9  run-time plan; the reference's default p at this rate
#   q8000x2    8 Msps   8000   2  4000  16000   9  packed default (variant 103), PRN groups
#   q12000x3   12 Msps  12000  3  4000  36000   9  odd p, nine segments, packed
#   q12000x2   12 Msps  12000  2  6000  24000   9  run-time plan
#   q25000x4   25 Msps  25000  4  6250  100000  5  the real 25 Msps shape; longest wipe-off and sums
CASES = {
    "q4000x2": dict(spc=4000, p=2, D=9),
    "q4000x4": dict(spc=4000, p=4, D=9),
    "q8000x2": dict(spc=8000, p=2, D=9),
    "q12000x3": dict(spc=12000, p=3, D=9),
    "q12000x2": dict(spc=12000, p=2, D=9),
    "q25000x4": dict(spc=25000, p=4, D=5),
}


class QuickCase:
    """The replicas, NITEMS items and their float64 records of one case."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.spc, self.p, self.D = name, c["spc"], c["p"], c["D"]
        self.fs, self.dstep = self.spc * 1000, 250
        self.nf, self.L = self.spc // self.p, self.p * self.spc
        self.dmax = (self.D - 1) // 2 * self.dstep
        rows = doppler_rows(self.dmax, self.dstep)
        assert len(rows) == self.D
        # (prn, present, row, tau)
        self.sats = [(1, True, 2, self.spc // 3 + 1), (4, True, self.D - 1, self.spc - 1),
                     (9, True, self.D // 2, self.nf + self.nf // 2), (7, False, 0, 0)]
        self.prns = [s[0] for s in self.sats]
        self.codes = np.stack([synth.gps_ca_sampled(prn, self.fs) for prn in self.prns]).astype(np.complex64)
        assert self.codes.shape == (len(self.prns), self.spc)
        amp = float(np.sqrt(200.0 * self.p / self.spc))
        x = np.zeros((NITEMS, self.L), np.complex128)
        n = np.arange(self.L)
        for q, (prn, present, row, tau) in enumerate(self.sats):
            if not present:
                continue
            code = self.codes[q].astype(np.complex128)[(n - tau) % self.spc]
            for b in range(NITEMS):
                x[b] += amp * code * np.exp(1j * (2 * np.pi * rows[row] * (n + b * self.L) / self.fs + 0.3 + q))
        rng = np.random.default_rng(synth.SEED + 7000 + self.spc + self.p)
        re = rng.standard_normal((NITEMS, self.L))
        im = rng.standard_normal((NITEMS, self.L))
        x += (re + 1j * im) * np.sqrt(0.5)
        self.x = x.astype(np.complex64)

    def items(self, item_type=0):
        """The items as the handle's type, and as the complex samples the engine reads."""
        flat = self.x.reshape(-1)
        if item_type == 0:
            return flat, self.x
        raw = synth.to_cshort(flat, 1000.0) if item_type == 1 else synth.to_ibyte(flat, 20.0)
        val = (raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)).reshape(self.x.shape)
        return raw, val

    @functools.lru_cache(maxsize=None)
    def reference(self, b, q, item_type=0, stamp0=0):
        x = self.items(item_type)[1][b]
        return item_record(x, self.fs, self.dmax, self.dstep, self.codes[q], self.p, stamp0 + b * self.L)


@functools.lru_cache(maxsize=None)
def quick_case(name):
    return QuickCase(name)


def capture_case():
    """The committed GPS capture (4 Msps, PRN 1): exactly one p = 2 item, +-10 kHz / 250 Hz."""
    return dict(fs=4000000, spc=4000, p=2, dmax=10000, dstep=250, code=synth.gps_ca_sampled(1, 4000000))

"""Float64 restatement of the two paired-code acquisition blocks and the inputs their tests share.

Written from the reference's text, not from the engine's formulation:
  pcps_cccwsr_acquisition_cc.cc
    :126-144  set_local_code(code_data, code_pilot): conj(FFT) of each;
    :250-252  d_input_power = sum |x|^2 / fft_size;
    :255-299  per Doppler row: FFT(x .* wipe-off), two inverse FFTs (data, pilot);
    :301-310  plus = (d.re - p.im, d.im + p.re), minus = (d.re + p.im, d.im - p.re), point by point;
    :312-320  index_max (first maximum) of |plus|^2 and |minus|^2, / (float(N) float(N))^2;
    :322-331  magt = plus if magt_plus >= magt_minus else minus;
    :334-341  if d_mag < magt: d_mag, Acq_delay_samples = indext % samples_per_code, Doppler, stamp, step;
    :360-370  d_test_statistics = d_mag / d_input_power; positive above the threshold, negative
              after max_dwells;
    :211-436  the state machine (0 stand-by, 1 one item per call, 2 / 3 publish 1 / 2).
  galileo_pcps_8ms_acquisition_cc.cc
    :114-135  code A = the code, code B = the code with samples [spc, 2 spc) negated;
    :238-239  d_input_power and d_mag zeroed in every state-1 call; the rest as above.
The Doppler wipe-off is the exact carrier exp(-j 2 pi f n / fs) (the engine's default model).
"""
import functools

import numpy as np

from gsdr import synth

MIN_MARGIN = 1e-3   # every comparison of an index, row or member first pins the winner this far above its runner-up
RTOL = 1e-4         # the project's acquisition tolerance, relative to the grid maximum
CCCWSR, PCPS_8MS = "cccwsr", "8ms"


def doppler_rows(dmax, dstep):
    """The bins init() counts (:160-166) and their frequencies (:257)."""
    return [-dmax + dstep * i for i in range(len(range(-dmax, dmax + 1, dstep)))]


def index_max(m):
    """volk_gnsssdr_32f_index_max_32u: the first maximum."""
    return int(np.argmax(m))


def input_power(x):
    x = np.asarray(x, np.complex128)
    return float(np.sum(x.real ** 2 + x.imag ** 2) / len(x))


def members_8ms(code, spc):
    """Code A and code B (galileo_pcps_8ms_acquisition_cc.cc:114-135)."""
    a = np.array(code, np.complex128)
    b = a.copy()
    b[spc:2 * spc] = -b[spc:2 * spc]
    return a, b


def _spectra(x, fs, dmax, dstep):
    x = np.asarray(x, np.complex128)
    n = np.arange(len(x), dtype=np.float64)
    for f in doppler_rows(dmax, dstep):
        yield np.fft.fft(x * np.exp(-2j * np.pi * ((f * n / fs) % 1.0)))


def _top2(m):
    two = np.partition(m, len(m) - 2)[len(m) - 2:]
    return float(two[1]), float(two[0])


def member_rows(x, fs, dmax, dstep, policy, first, second, spc=None):
    """-> mags [D, 2], idx [D, 2], idx_margin [D, 2]: per Doppler row the two members' normalised
    maxima (magt_plus / magt_minus, or magt_A / magt_B), their first-maximum indices and
    (best - second best) / best inside each member's row.

    The 8 ms block's code A is periodic and its code B antiperiodic in samples_per_code, so
    |R[n + spc]| = |R[n]| in exact arithmetic: every row holds its maximum twice, and which of the
    two cells index_max meets first is a matter of rounding in the reference too.  What the block
    publishes is indext % samples_per_code (:337), which does not depend on it; so for that policy
    the index margin is taken over the delays n % spc, and the tests compare code_phase mod spc."""
    N = len(x)
    norm = (float(N) * float(N)) ** 2
    f0 = np.conj(np.fft.fft(np.asarray(first, np.complex128)))
    f1 = np.conj(np.fft.fft(np.asarray(second, np.complex128)))
    mags, idx, marg = [], [], []
    for X in _spectra(x, fs, dmax, dstep):
        r0 = np.fft.ifft(X * f0) * N  # the unnormalised inverse transform
        r1 = np.fft.ifft(X * f1) * N
        if policy == CCCWSR:
            plus = (r0.real - r1.imag) + 1j * (r0.imag + r1.real)
            minus = (r0.real + r1.imag) + 1j * (r0.imag - r1.real)
            pair = (plus, minus)
        else:
            pair = (r0, r1)
        mm, ii, gg = [], [], []
        for c in pair:
            m = c.real ** 2 + c.imag ** 2
            i = index_max(m)
            fold = m.reshape(-1, spc).max(axis=0) if policy == PCPS_8MS and spc and len(m) % spc == 0 else m
            best, nxt = _top2(fold)
            mm.append(m[i] / norm)
            ii.append(i)
            gg.append((best - nxt) / best)
        mags.append(mm)
        idx.append(ii)
        marg.append(gg)
    return np.array(mags), np.array(idx), np.array(marg)


def grid_decide(mags, idx, spc, dmax, dstep):
    """:322-341 over the rows of one item, from d_mag = 0 -> dict."""
    d_mag, out = 0.0, None
    rows = doppler_rows(dmax, dstep)
    for d in range(len(rows)):
        if mags[d, 0] >= mags[d, 1]:
            magt, indext, member = mags[d, 0], idx[d, 0], 0
        else:
            magt, indext, member = mags[d, 1], idx[d, 1], 1
        if d_mag < magt:
            d_mag = magt
            out = dict(doppler_index=d, code_phase=int(indext), member=member, doppler_hz=rows[d],
                       acq_delay_samples=float(int(indext) % int(spc)), mag=float(magt))
    return out


def margins(mags, idx_margin, win):
    """Row, member and index margins of a decided grid, each (winner - runner-up) / winner."""
    d, m = win["doppler_index"], win["member"]
    rowmax = mags.max(axis=1)
    others = np.delete(rowmax, d)
    row = (rowmax[d] - others.max()) / rowmax[d] if len(others) else 1.0
    member = abs(mags[d, 0] - mags[d, 1]) / rowmax[d]
    return dict(row=float(row), member=float(member), index=float(idx_margin[d, m]))


def block_record(x, fs, dmax, dstep, policy, first, second, spc, stamp):
    """One item's grid: the record gsdr_acq_run_pairs owes, the rows and the margins."""
    mags, idx, im = member_rows(x, fs, dmax, dstep, policy, first, second, spc)
    win = grid_decide(mags, idx, spc, dmax, dstep)
    ip = input_power(x)
    win.update(input_power=ip, test_statistic=win["mag"] / ip, samplestamp=int(stamp))
    return dict(rec=win, mags=mags, idx=idx, margins=margins(mags, im, win))


def decide(records, threshold, carry_mag):
    """The dwell rule over one satellite's per-item records (dicts of block_record) ->
    (record, positive, num_dwells): the state-1 calls of :238-370 one after the other."""
    d_mag, held = 0.0, None
    for k, r in enumerate(records):
        if not carry_mag:
            d_mag, held = 0.0, held  # the synchro fields are not cleared, only d_mag (:238-239)
        if d_mag < r["mag"]:
            d_mag, held = r["mag"], r
        out = dict(held)
        out.update(mag=d_mag, input_power=r["input_power"], test_statistic=d_mag / r["input_power"])
        if out["test_statistic"] > threshold:
            return out, True, k + 1
    return out, False, len(records)


class RefBlock:
    """general_work of both blocks (:205-436) over items of fft_size samples."""

    def __init__(self, policy, fs, N, spc, dmax, dstep, max_dwells, threshold, first, second):
        self.policy, self.fs, self.N, self.spc, self.dmax, self.dstep = policy, fs, N, spc, dmax, dstep
        self.max_dwells, self.threshold, self.first, self.second = max_dwells, threshold, first, second
        self.state, self.active, self.sample_counter, self.well_count = 0, False, 0, 0
        self.mag = self.ip = self.stat = 0.0
        self.synchro = dict(acq_delay_samples=0.0, acq_doppler_hz=0.0, acq_samplestamp_samples=0, acq_doppler_step=0)

    def _restart(self):
        self.synchro = dict(acq_delay_samples=0.0, acq_doppler_hz=0.0, acq_samplestamp_samples=0, acq_doppler_step=0)
        self.well_count, self.mag, self.ip, self.stat = 0, 0.0, 0.0, 0.0

    def work(self, items):
        """items: the ninput_items items offered -> (consumed, event)."""
        n, event = len(items), 0
        if self.state == 0:
            if self.active:
                self._restart()
                self.state = 1
            self.sample_counter += self.N * n
            return n, 0
        if self.state == 1:
            if self.policy == PCPS_8MS:
                self.ip = self.mag = 0.0
            self.sample_counter += self.N
            self.well_count += 1
            b = block_record(items[0], self.fs, self.dmax, self.dstep, self.policy, self.first, self.second, self.spc, 0)
            self.ip = b["rec"]["input_power"]
            if self.mag < b["rec"]["mag"]:
                self.mag = b["rec"]["mag"]
                self.synchro = dict(acq_delay_samples=b["rec"]["acq_delay_samples"],
                                    acq_doppler_hz=float(b["rec"]["doppler_hz"]),
                                    acq_samplestamp_samples=self.sample_counter, acq_doppler_step=self.dstep)
            self.stat = self.mag / self.ip
            if self.stat > self.threshold:
                self.state = 2
            elif self.well_count == self.max_dwells:
                self.state = 3
            return 1, 0
        event = 1 if self.state == 2 else 2
        self.active = False
        self.state = 0
        self.sample_counter += self.N * n
        return n, event


def run_attempts(block, x, attempts, per_call=1):
    """The self-test driver's loop (host/tests/pair_acquisition_selftest.cc) on a RefBlock."""
    N, offset, out = block.N, 0, []
    for _ in range(attempts):
        block.active = True
        calls, event = [], 0
        while event == 0 and offset + N <= len(x):
            offered = min(per_call, (len(x) - offset) // N)
            state = block.state
            c, event = block.work([x[offset + i * N:offset + (i + 1) * N] for i in range(offered)])
            offset += c * N
            calls.append(dict(state=state, offered=offered, consumed=c, event=event, mag=block.mag,
                              input_power=block.ip, test_statistic=block.stat, **block.synchro))
        out.append(dict(calls=calls, event=event, end_state=block.state, sample_counter=block.sample_counter))
    return out


def threshold_8ms(pfa, vector_length, dmax, dstep):
    """galileo_e1_pcps_8ms_ambiguous_acquisition.cc:239-257 (pfa is a float there)."""
    ncells = vector_length * len(doppler_rows(dmax, dstep))
    val = (1.0 - float(np.float32(pfa))) ** (1.0 / ncells)
    return float(np.float32(-np.log1p(-val) / float(vector_length)))


def sampled_ms_key(value):
    """coherent_integration_time_ms as the adapters round it (:59-67)."""
    return value if value % 4 == 0 else (value // 4) * 4


# ---------------------------------------------------------------- signals
def member_signal(B, C, tau, d, s, doppler_hz, fs, amp, seed, noise=1.0, n0=0):
    """amp (d B[n - tau] + j s C[n - tau]) carrier + noise: minus (member 1) wins when d = s,
    plus (member 0) when d = -s, and the other member is near zero."""
    N = len(B)
    rng = np.random.default_rng(synth.SEED + 4000 + seed)
    n = np.arange(N, dtype=np.float64) + n0
    sig = amp * (d * np.roll(B, tau) + 1j * s * np.roll(C, tau)) * np.exp(2j * np.pi * doppler_hz * n / fs)
    return sig + noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.5)


def bits_signal(code, spc, tau, bits, doppler_hz, fs, amp, seed, noise=1.0, phase=0.3):
    """E1-B alone over an item of two code periods: bits = (before tau, first period, second
    period).  (1, 1, 1) is code A's case; (-1, 1, -1) code B's: a data-bit edge between the
    two periods."""
    N = 2 * spc
    c = np.asarray(code[:spc], np.complex128)
    n = np.arange(N)
    b = np.where(n < tau, bits[0], np.where(n < tau + spc, bits[1], bits[2]))
    rng = np.random.default_rng(synth.SEED + 5000 + seed)
    sig = amp * b * c[(n - tau) % spc] * np.exp(1j * (2 * np.pi * doppler_hz * n / fs + phase))
    return sig + noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.5)


def codes_for(prn, spc, N):
    """E1-B and E1-C replicas of spc samples per 4 ms period, in rows of N: one period and
    zeros behind it, as the CCCWSR adapter leaves its buffers (:76-77, :185-205)."""
    fs = spc * 250
    out = []
    for pilot in (False, True):
        row = np.zeros(N, np.complex64)
        row[:spc] = synth.gal_e1_sampled(prn, fs, pilot=pilot)[:spc]
        out.append(row)
    return out


# One case per FFT plan and kind.  sats: (prn, present, row, tau, which member is meant to win).
#   N      path                                   rows
#   2000   compile-time LDS plan                  9
#   4000   default packed variant, 9 pairs = 18 slots: pair 8 is a PRN group of its own   9
#   6000   run-time plan                          9
#   16000  register four-step (CCCWSR's size at 4 Msps)   9
#   32000  split (the 8 ms block's size at 4 Msps)        5
NBLOCKS = 3
CASES = {}
for _N, _D in ((2000, 9), (4000, 9), (6000, 9), (16000, 9), (32000, 5)):
    _sats = [(1, True, 2, _N // 3 + 1, 1), (4, True, _D - 2, _N - 1, 0), (7, False, 0, 0, 0)]
    if _N == 4000:
        _sats = [(1, True, 2, 1334, 1), (2, False, 0, 0, 0), (3, True, 0, 0, 0), (4, True, 7, 3999, 0),
                 (5, False, 0, 0, 0), (6, True, 8, 1, 1), (7, False, 0, 0, 0), (8, True, 4, 2000, 0),
                 (9, True, 5, 77, 1)]
    CASES["sdj%d" % _N] = dict(policy=CCCWSR, N=_N, spc=_N, D=_D, sats=_sats)
    CASES["asis%d" % _N] = dict(policy=PCPS_8MS, N=_N, spc=_N // 2, D=_D, sats=_sats[:3] if _N != 4000 else _sats)


class PairCase:
    """The replicas, NBLOCKS items and their float64 records of one case."""

    def __init__(self, name):
        c = CASES[name]
        self.name, self.policy, self.N, self.spc, self.D = name, c["policy"], c["N"], c["spc"], c["D"]
        self.fs, self.dstep = self.spc * 250, 250
        self.dmax = (self.D - 1) // 2 * self.dstep
        assert len(doppler_rows(self.dmax, self.dstep)) == self.D
        self.prns = [s[0] for s in c["sats"]]
        # the amplitude that puts a present satellite's statistic near 0.5 at every size
        amp = float(np.sqrt(1.0 / (0.004 * self.fs) * 40.0))
        rows = doppler_rows(self.dmax, self.dstep)
        self.first, self.second = [], []
        x = np.zeros((NBLOCKS, self.N), np.complex128)
        for q, (prn, present, row, tau, member) in enumerate(c["sats"]):
            B, C = codes_for(prn, self.spc, self.N)
            if self.policy == CCCWSR:
                self.first.append(B)
                self.second.append(C)
            else:
                code = np.tile(B[:self.spc], 2)
                self.first.append(code)
                self.second.append(members_8ms(code, self.spc)[1].astype(np.complex64))
            if not present:
                continue
            for b in range(NBLOCKS):
                if self.policy == CCCWSR:
                    s = 1.0 if member == 1 else -1.0
                    x[b] += member_signal(B.astype(np.complex128), C.astype(np.complex128), tau, 1.0, s, rows[row], self.fs,
                                          amp, seed=0, noise=0.0, n0=b * self.N)
                else:
                    bits = (-1, 1, -1) if member == 1 else (1, 1, 1)
                    x[b] += bits_signal(B, self.spc, tau % self.spc, bits, rows[row], self.fs, amp * 1.4, seed=0, noise=0.0,
                                        phase=0.3 + q)
        rng = np.random.default_rng(synth.SEED + 6000 + self.N + (1 if self.policy == CCCWSR else 2))
        x += (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)) * np.sqrt(0.5)
        self.x = x.astype(np.complex64)
        self.first = np.stack(self.first).astype(np.complex64)
        self.second = np.stack(self.second).astype(np.complex64)

    @property
    def kind(self):
        import gsdr
        return gsdr.PAIR_SUM_DIFF_J if self.policy == CCCWSR else gsdr.PAIR_AS_IS

    def args(self):
        """What set_code_pairs gets: the reference's own arguments (CCCWSR: data and pilot;
        8 ms: code A and code B as set_local_code forms them)."""
        return self.kind, self.first, self.second, np.array(self.prns, np.uint32)

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
        return block_record(x, self.fs, self.dmax, self.dstep, self.policy, self.first[q], self.second[q], self.spc,
                            stamp0 + b * self.N)


@functools.lru_cache(maxsize=None)
def pair_case(name):
    return PairCase(name)


def capture_case(cap, policy):
    """The committed Galileo capture (4 Msps, PRN 1), +-10 kHz / 250 Hz: CCCWSR on 16000-sample
    items, the 8 ms block on the whole 32000."""
    B, C = codes_for(1, 16000, 16000)
    if policy == CCCWSR:
        return dict(fs=4000000, N=16000, spc=16000, dmax=10000, dstep=250, first=B, second=C)
    code = np.tile(B, 2)
    return dict(fs=4000000, N=32000, spc=16000, dmax=10000, dstep=250, first=code,
                second=members_8ms(code, 16000)[1].astype(np.complex64))

"""Float64 restatement of the Tong acquisition block and the inputs its tests share.

Written from the reference's text, not from the engine's formulation:
  pcps_tong_acquisition_cc.cc
    :81, :105  an item is N = sampled_ms * samples_per_ms samples; d_fft_size = N;
    :142-150   set_local_code: conj(FFT(code));
    :166-184   the Doppler rows: -doppler_max + step i while <= doppler_max; the wipe-off of row i;
    :188-218   set_state(1): d_dwell_count = 0, d_tong_count = tong_init_val, the grid and the synchro
               fields zeroed;
    :229-258   state 0: the same restart when d_active, then state 1; everything offered is consumed;
    :261-376   state 1, one item per call:
      :268       fft_normalization_factor = float(N) float(N);
      :269-274   d_input_power = d_mag = 0; d_sample_counter += N before the grid; d_dwell_count++;
      :283-285   d_input_power = sum |x|^2 / N;
      :293-309   per row: |IFFT(FFT(x w_d) C)|^2, unnormalised transforms;
      :312-314   times 1 / (fn fn d_input_power);
      :317       added into d_grid_data[d];
      :320-322   indext = the first maximum of the accumulated row, magt its value;
      :325-332   if d_mag < magt the row takes over: Acq_delay_samples = indext % samples_per_code,
                 Acq_doppler_hz, Acq_samplestamp_samples = d_sample_counter, Acq_doppler_step;
      :350-372   d_test_statistics = d_mag; above threshold * d_dwell_count the count goes up and
                 the block is positive (state 2) when it equals tong_max_val, else it goes down and
                 the block is negative (state 3) at zero; then d_dwell_count >= tong_max_dwells
                 makes it negative whatever came before;
    :378-436   states 2 and 3: event 1 or 2, everything offered consumed, back to state 0; state 2
               also writes the monitor output.
  gps_l1_ca_pcps_tong_acquisition.cc :226-245 and
  galileo_e1_pcps_tong_ambiguous_acquisition.cc :247-266: calculate_threshold.
The Doppler wipe-off is the exact carrier exp(-j 2 pi f n / fs) (the engine's default model).
"""
import functools

import numpy as np

from gsdr import synth

MIN_MARGIN = 1e-3      # every winner (row, index) is first pinned this far above its runner-up
MIN_DECISION = 0.05    # every statistic is this far from threshold * dwell, relative to the latter
RTOL = 1e-4            # the project's acquisition tolerance
RUNNING, POSITIVE, NEGATIVE, PAST_END = 0, 1, 2, 3


def doppler_rows(dmax, dstep):
    """The bins init() counts (:166-173) and their frequencies (:180)."""
    return [-dmax + dstep * i for i in range(len(range(-dmax, dmax + 1, dstep)))]


def input_power(x):
    x = np.asarray(x, np.complex128)
    return float(np.sum(x.real ** 2 + x.imag ** 2) / len(x))


def wipeoff(f, fs, n):
    k = np.arange(n, dtype=np.float64)
    return np.exp(-2j * np.pi * ((f * k / fs) % 1.0))


def item_rows(x, fs, rows, code):
    """:283-314 -> [D, N]: an item's rows, scaled by the item's own input power."""
    x = np.asarray(x, np.complex128)
    n = len(x)
    assert len(code) == n
    cf = np.conj(np.fft.fft(np.asarray(code, np.complex128)))
    fn = float(n) * float(n)
    scale = 1.0 / (fn * fn * input_power(x))
    out = np.empty((len(rows), n))
    for d, f in enumerate(rows):
        r = np.fft.ifft(np.fft.fft(x * wipeoff(f, fs, n)) * cf) * n  # the unnormalised inverse transform
        out[d] = (r.real ** 2 + r.imag ** 2) * scale
    return out


def accumulated(items, fs, rows, code):
    """:317 -> the grid after each item of a sequence that starts at items[0]."""
    grid = np.zeros((len(rows), len(items[0])))
    out = []
    for x in items:
        grid = grid + item_rows(x, fs, rows, code)
        out.append(grid)
    return out


def winner(grid):
    """:320-332 from d_mag = 0 -> (row, indext, d_mag, margin): rows ascending with strict '<', the first
    maximum in the row; margin = (winner - best other cell) / winner."""
    d_mag, row, idx = 0.0, None, None
    for d in range(grid.shape[0]):
        i = int(np.argmax(grid[d]))
        if d_mag < grid[d, i]:
            d_mag, row, idx = float(grid[d, i]), d, i
    flat = grid.reshape(-1).copy()
    flat[row * grid.shape[1] + idx] = -1.0
    return row, idx, d_mag, float((d_mag - flat.max()) / d_mag)


def counter(stats, threshold, init, tmax, max_dwells):
    """:350-372 over one sequence's statistics -> per statistic (dwell_count, tong_count, state, margin);
    past the terminal one PAST_END with the final counts.  margin = |stat - threshold dwell| /
    (threshold dwell)."""
    dwell, count, state, out = 0, init, RUNNING, []
    for s in stats:
        if state != RUNNING:
            out.append((dwell, count, PAST_END, None))
            continue
        dwell += 1
        if s > threshold * dwell:
            count += 1
            if count == tmax:
                state = POSITIVE
        else:
            count -= 1
            if count == 0:
                state = NEGATIVE
        if dwell >= max_dwells:
            state = NEGATIVE
        out.append((dwell, count, state, abs(s - threshold * dwell) / (threshold * dwell)))
    return out


def sequence_records(items, fs, dmax, dstep, code, spc, threshold, init, tmax, max_dwells, stamp0=0, prn=0):
    """What gsdr_acq_run_tong owes for one slot over a sequence that starts at items[0] -> (records,
    grids): a dict per item, and the accumulated grid after each item."""
    rows = doppler_rows(dmax, dstep)
    n = len(items[0])
    grids = accumulated(items, fs, rows, code)
    wins = [winner(g) for g in grids]
    cnt = counter([w[2] for w in wins], threshold, init, tmax, max_dwells)
    recs = []
    for k, (w, c) in enumerate(zip(wins, cnt)):
        r = dict(prn=prn, samplestamp=stamp0 + k * n, input_power=input_power(items[k]), dwell_count=c[0],
                 tong_count=c[1], state=c[2], doppler_index=0, indext=0, doppler_hz=0, acq_delay_samples=0.0, mag=0.0,
                 pad=0, winner_margin=None, decision_margin=None)
        if c[2] != PAST_END:
            r.update(doppler_index=w[0], indext=w[1], doppler_hz=rows[w[0]], acq_delay_samples=float(w[1] % spc),
                     mag=w[2], winner_margin=w[3], decision_margin=c[3])
        recs.append(r)
    return recs, grids


def threshold(pfa, vector_length, bins):
    """calculate_threshold: pfa a float, 1.0 - pfa a double, ncells an unsigned product, the exponential
    quantile -log1p(-val) / lambda with lambda = vector_length, cast to float."""
    ncells = vector_length * bins
    val = (1.0 - float(np.float32(pfa))) ** (1.0 / float(ncells))
    return float(np.float32(-np.log1p(-val) / float(vector_length)))


class RefBlock:
    """general_work (:221-440) over items of N samples.  stat_of: item index within the sequence and
    item -> (mag, delay, doppler_hz) of the accumulated grid, for driving the state machine on given
    statistics; by default the grid of this module."""

    def __init__(self, fs, n, spc, dmax, dstep, threshold, init, tmax, max_dwells, code=None, stat_of=None,
                 monitor=False, batch=1):
        self.fs, self.n, self.spc, self.dmax, self.dstep = fs, n, spc, dmax, dstep
        self.threshold, self.init, self.tmax, self.max_dwells = threshold, init, tmax, max_dwells
        self.code, self.stat_of, self.monitor, self.batch = code, stat_of, monitor, batch
        self.rows = doppler_rows(dmax, dstep)
        self.state, self.active, self.sample_counter = 0, False, 0
        self.dwell_count, self.tong_count = 0, init
        self.mag = self.ip = self.stat = 0.0
        self.grid, self.margin = None, None  # margin: the last dwell's winner over its runner-up
        self._restart()

    def _restart(self):
        self.synchro = dict(acq_delay_samples=0.0, acq_doppler_hz=0.0, acq_samplestamp_samples=0, acq_doppler_step=0)
        self.dwell_count, self.tong_count = 0, self.init
        self.mag = self.ip = self.stat = 0.0
        self.grid = None if self.code is None else np.zeros((len(self.rows), self.n))

    def set_state(self, state):
        self.state = state
        if state == 1:
            self._restart()

    def _dwell(self, item):
        """One state-1 call (:261-376)."""
        self.ip = self.mag = 0.0
        self.sample_counter += self.n
        self.dwell_count += 1
        if self.stat_of is not None:
            mag, delay, dop = self.stat_of(self.dwell_count - 1, item)
        else:
            self.grid = self.grid + item_rows(item, self.fs, self.rows, self.code)
            row, idx, mag, self.margin = winner(self.grid)
            delay, dop = float(idx % self.spc), float(self.rows[row])
            self.ip = input_power(item)
        if self.mag < mag:
            self.mag = mag
            self.synchro = dict(acq_delay_samples=delay, acq_doppler_hz=dop,
                                acq_samplestamp_samples=self.sample_counter, acq_doppler_step=self.dstep)
        self.stat = self.mag
        if self.stat > self.threshold * self.dwell_count:
            self.tong_count += 1
            if self.tong_count == self.tmax:
                self.state = 2
        else:
            self.tong_count -= 1
            if self.tong_count == 0:
                self.state = 3
        if self.dwell_count >= self.max_dwells:
            self.state = 3

    def work(self, items):
        """items: the ninput_items items offered -> (consumed, event, monitor output or None)."""
        n = len(items)
        if self.state == 0:
            if self.active:
                self._restart()
                self.state = 1
            self.sample_counter += self.n * n
            return n, 0, None
        if self.state == 1:
            # the reference takes one item per call (batch 1); the engine's block takes up to `batch`
            # and stops behind the item that ends the sequence: as many reference calls in one
            left = max(self.max_dwells - self.dwell_count, 1)
            used = 0
            while used < min(n, self.batch, left) and self.state == 1:
                self._dwell(items[used])
                used += 1
            return used, 0, None
        event = 1 if self.state == 2 else 2
        out = dict(self.synchro) if (self.state == 2 and self.monitor) else None
        self.active = False
        self.state = 0
        self.sample_counter += self.n * n
        return n, event, out


def block_decisions(stats, threshold, init, tmax, max_dwells):
    """RefBlock driven one item per call on the given statistics -> per statistic (dwell_count, tong_count,
    state as the engine's records name it); PAST_END once the block has left state 1."""
    b = RefBlock(1000, 1, 1, 0, 1, threshold, init, tmax, max_dwells, stat_of=lambda k, item: (stats[k], 0.0, 0.0))
    b.set_state(1)
    out = []
    for k in range(len(stats)):
        if b.state != 1:
            out.append((b.dwell_count, b.tong_count, PAST_END))
            continue
        b.work([None])
        out.append((b.dwell_count, b.tong_count, {1: RUNNING, 2: POSITIVE, 3: NEGATIVE}[b.state]))
    return out


def run_attempts(block, x, attempts, per_call=1):
    """The self-test driver's loop (host/tests/tong_acquisition_selftest.cc) on a RefBlock: per attempt
    d_active is raised and work() is called on what is left of x, per_call items at most, until an event."""
    n, offset, out = block.n, 0, []
    for _ in range(attempts):
        block.active = True
        calls, event = [], 0
        while event == 0 and offset + n <= len(x):
            offered = min(per_call, (len(x) - offset) // n)
            state = block.state
            c, event, mon = block.work([x[offset + i * n:offset + (i + 1) * n] for i in range(offered)])
            offset += c * n
            calls.append(dict(state=state, offered=offered, consumed=c, event=event, mag=block.mag,
                              input_power=block.ip, dwell_count=block.dwell_count, tong_count=block.tong_count,
                              monitor=mon, winner_margin=block.margin, **block.synchro))
        out.append(dict(calls=calls, event=event, end_state=block.state, sample_counter=block.sample_counter))
    return out


# ---------------------------------------------------------------- the shared cases
# One-millisecond items at fs = 1000 N, nine rows of 250 Hz, tong_init_val 2, tong_max_val 4,
# tong_max_dwells 8, threshold THRESHOLD, two streams of eight items with three code slots each.  A
# satellite's entry gives, per item, the contribution c_k of that item to the accumulated grid at the
# satellite's own cell in units of the threshold (0: absent from the item); its statistic after k
# items is S_k = c_1 + ... + c_k plus what noise and the other satellites leave in that cell, compared
# with k.  The amplitudes are solved per item so that the float64 restatement meets c_k.
#
#   stream 1  slot 0  PRN 1  row 2, delay N/3+1   c = 3 3 0 0 0 0 0 0     up up: positive after two dwells
#             slot 1  PRN 7  absent                                       down down: negative after two
#             slot 2  PRN 4  row 8, delay N-1     S/k = 1.5 .75 .5 1.1 1.09 .91 .78 1.1
#                                                 u d d u u d d u: running count 2 when tong_max_dwells cuts it
#   stream 2  slot 0  PRN 9  row 4, delay N/2+3   S/k = 0 1.15 1.14 .86 .68 1.15 1.15 1.15
#                                                 d u u d d u u u: count 4 on dwell 8, the overridden positive
#             slot 1  PRN 12 row 0, delay 1       S/k = 1.3 .65 1.17 1.18: up down up up, positive after four
#             slot 2  PRN 9's code again, under the id 31: records equal to slot 0's apart from the prn
#
#   case    N      plan
#   t2000   2000   compile-time, row in LDS
#   t4000   4000   compile-time; the handle's plain search is packed (variant 103)
#   t3000   3000   run-time, row in LDS
#   t16000  16000  compile-time, 1024 lanes; the row does not fit beside the transform: kept in HBM
THRESHOLD, INIT, TMAX, MAX_DWELLS, NITEMS, D, DSTEP = 0.05, 2, 4, 8, 8, 9, 250
SEED_OFFSET = 9002  # one for which every noise-only winner meets MIN_MARGIN as well
CASES = {"t2000": 2000, "t4000": 4000, "t3000": 3000, "t16000": 16000}


def _streams(n):
    return [
        dict(slots=[1, 7, 4], code_of=[1, 7, 4],
             sats={1: dict(row=2, tau=n // 3 + 1, c=[3, 3, 0, 0, 0, 0, 0, 0]),
                   4: dict(row=D - 1, tau=n - 1, c=[1.5, 0, 0, 2.9, 1.05, 0, 0, 3.4])}),
        dict(slots=[9, 12, 31], code_of=[9, 12, 9],
             sats={9: dict(row=D // 2, tau=n // 2 + 3, c=[0, 2.3, 1.12, 0, 0, 3.48, 1.15, 1.15]),
                   12: dict(row=0, tau=1, c=[1.3, 0, 2.2, 1.2, 0, 0, 0, 0])}),
    ]


def _cell(x, w, code, tau, n):
    """An item's scaled contribution at (the row of wipe-off w, delay tau): :293-314 at one cell."""
    t = (x * w)[(np.arange(n) + tau) % n]
    r = np.sum(t * np.conj(code))
    return (r.real ** 2 + r.imag ** 2) / (float(n) * float(n) * input_power(x))


class TongCase:
    """The replicas and items of both streams of one case, and their float64 records."""

    def __init__(self, name):
        self.name, self.n = name, CASES[name]
        n = self.n
        self.fs, self.spc, self.dstep, self.D = 1000 * n, n, DSTEP, D
        self.dmax = (D - 1) // 2 * DSTEP
        self.rows = doppler_rows(self.dmax, self.dstep)
        assert len(self.rows) == D
        self.streams = _streams(n)
        rng = np.random.default_rng(synth.SEED + SEED_OFFSET + n)
        idx = np.arange(n)
        for st in self.streams:
            st["codes"] = np.stack([synth.gps_ca_sampled(p, self.fs) for p in st["code_of"]]).astype(np.complex64)
            assert st["codes"].shape == (len(st["slots"]), n)
            noise = (rng.standard_normal((NITEMS, n)) + 1j * rng.standard_normal((NITEMS, n))) * np.sqrt(0.5)
            x = np.empty((NITEMS, n), np.complex128)
            for k in range(NITEMS):
                sig = {}
                for q, (prn, s) in enumerate(st["sats"].items()):
                    code = synth.gps_ca_sampled(prn, self.fs).astype(np.complex128)
                    s["code"], s["w"] = code, wipeoff(self.rows[s["row"]], self.fs, n)
                    sig[prn] = code[(idx - s["tau"]) % n] * np.exp(
                        1j * (2 * np.pi * self.rows[s["row"]] * (idx + k * n) / self.fs + 0.3 + q))
                amp = {prn: np.sqrt(s["c"][k] * THRESHOLD) for prn, s in st["sats"].items()}
                for _ in range(6):  # fixed point: the cell's value moves as the amplitude squared
                    xk = noise[k] + sum(amp[p] * sig[p] for p in sig)
                    for prn, s in st["sats"].items():
                        if s["c"][k] > 0:
                            amp[prn] *= np.sqrt(s["c"][k] * THRESHOLD / _cell(xk, s["w"], s["code"], s["tau"], n))
                x[k] = noise[k] + sum(amp[p] * sig[p] for p in sig)
            st["x"] = x.astype(np.complex64)

    def items(self, stream, item_type=0):
        """The stream's items as the handle's type, and as the complex samples the engine reads."""
        x = self.streams[stream]["x"]
        flat = x.reshape(-1)
        if item_type == 0:
            return flat, x
        raw = synth.to_cshort(flat, 1000.0) if item_type == 1 else synth.to_ibyte(flat, 20.0)
        val = (raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)).reshape(x.shape)
        return raw, val

    @functools.lru_cache(maxsize=None)
    def reference(self, stream, slot, first=0, count=NITEMS, item_type=0, stamp0=0):
        """(records, grids) of a sequence of the slot that starts at item `first` of the stream."""
        st = self.streams[stream]
        x = self.items(stream, item_type)[1]
        return sequence_records([x[k] for k in range(first, first + count)], self.fs, self.dmax, self.dstep,
                                st["codes"][slot], self.spc, THRESHOLD, INIT, TMAX, MAX_DWELLS, stamp0,
                                st["slots"][slot])


@functools.lru_cache(maxsize=None)
def tong_case(name):
    return TongCase(name)


def assert_margins(recs):
    """The conditions every comparison with the engine rests on: asserted on the restatement alone."""
    for k, r in enumerate(recs):
        if r["state"] == PAST_END:
            continue
        assert r["winner_margin"] >= MIN_MARGIN, (k, r)
        assert r["decision_margin"] >= MIN_DECISION, (k, r)


def capture_case():
    """The committed GPS capture (4 Msps, PRN 1): two 1 ms items, +-10 kHz / 250 Hz."""
    return dict(fs=4000000, n=4000, spc=4000, dmax=10000, dstep=250, code=synth.gps_ca_sampled(1, 4000000))

"""Scenarios of the Galileo E5a (5X) / GPS L5 tracking tests (not a test module), shared by
test_trk_restatement.py (the restatement alone, no GPU) and test_gpu_trk_wideband.py.

One satellite, 45 dB-Hz over both components, pull_in_time_s 0 (the transitory ends after
one second, call 1000), 1.3 s of input.  The E5a primary chips come from
iq_caf_checks.e5a_random_table, the GPS L5 ones and the per-PRN E5a-Q secondary codes are
seeded random: the engine takes any replica and ships no E5a table.

Below the 10.23 Mcps chip rate a sample spans more than one chip (2.56 chips at 4 Msps), and
start_tracking begins the first call at a whole sample with a zero code remainder
(dll_pll_veml_tracking.cc:1813-1844), so an acquisition can be off by half a sample, more
than the correlation peak is wide.  The scenarios therefore put the satellite's code start
0.1 chip away from a whole sample, which is what "the acquisition found it" means at these
rates.  Started at nitems_read 0 the pull-in call skips to the second code start, so
call k correlates code epoch k + 1; the transitory ends at call 999 (epoch 1000), so the
secondary codes (100, 20 or 10 symbols, index = epoch mod length) line up with the first
full buffer: bit synchronisation at call 999 + length - 1.

The carrier phase (3.2 rad at 4 Msps, 2.7 rad at 5 Msps: PHASE) is chosen so that the two-quadrant PLL of state 2 settles
with the prompt positive on secondary chip '0'.  That is the polarity acquire_secondary
reports as Flag_PLL_180_deg_phase_locked (:923-967) and the one on which the wiped
prompt of state 4 is already positive; from the other one the four-quadrant PLL of pilot
tracking turns the carrier by half a cycle during the first data bit after bit
synchronisation, and that bit comes out with the opposite sign of all later ones.
"""
import functools

import numpy as np

import gsdr
from gsdr import synth

import iq_caf_checks
from trk_checks import _conf_sig

SECONDS = 1.3
PHASE = {4.0e6: 3.2, 5.0e6: 2.7}  # carrier phase of the satellite per sampling rate (see above)
CHIP_RATE = 1.023e7
CARRIER_HZ = 1.17645e9
CASES = [("5X", 1), ("5X", 0), ("L5", 1), ("L5", 0)]
SIGNAL = {"5X": gsdr.SIGNAL_GAL_5X, "L5": gsdr.SIGNAL_GPS_L5}
SYMBOLS_PER_BIT = {"5X": 20, "L5": 10}
# d_interchange_iq (dll_pll_veml_tracking.cc:242, :310)
SWAP = {("5X", 1): True, ("5X", 0): False, ("L5", 1): False, ("L5", 0): True}
# the secondary code bit synchronisation searches for: its length
SYNC_LEN = {("5X", 1): 100, ("5X", 0): 20, ("L5", 1): 20, ("L5", 0): 10}


@functools.lru_cache(maxsize=None)
def _e5a_table():
    return iq_caf_checks.e5a_random_table(17)


def e5a_secondary(prn):
    """A 100-chip '0'/'1' stand-in for the PRN's E5a-Q secondary code."""
    return "".join("01"[b] for b in np.random.default_rng(synth.SEED + 500 + prn).integers(0, 2, 100))


def primary_codes(system, prn):
    """(data component chips, pilot component chips), +-1 float32."""
    if system == "5X":
        t = _e5a_table()
        return (iq_caf_checks.e5a_chips(t, prn, "I").astype(np.float32), iq_caf_checks.e5a_chips(t, prn, "Q").astype(np.float32))
    r = np.random.default_rng(synth.SEED + 700 + prn)
    return (1.0 - 2.0 * r.integers(0, 2, 10230)).astype(np.float32), (1.0 - 2.0 * r.integers(0, 2, 10230)).astype(np.float32)


def satellite(system, prn, fs, doppler_hz, start_sample, cn0=45.0, phase=3.2):
    """A satellite whose code epoch 0 starts 0.1 chip after input sample start_sample."""
    ci, cq = primary_codes(system, prn)
    chips_per_sample = CHIP_RATE * (1.0 + doppler_hz / CARRIER_HZ) / fs
    return synth.WidebandSatellite(prn, doppler_hz, start_sample * chips_per_sample + 0.1, ci, cq,
                                   e5a_secondary(prn) if system == "5X" else None, cn0, phase)


class Case:
    """One signal/mode at one rate: input, configuration and what start() takes."""

    def __init__(self, system, pilot, fs, seconds=SECONDS, prn=11, doppler_hz=1234.5, start_sample=1357, item=None):
        self.system, self.pilot, self.fs, self.prn = system, pilot, fs, prn
        self.sat = satellite(system, prn, fs, doppler_hz, start_sample, phase=PHASE.get(fs, 3.2))
        self.n = int(seconds * fs)
        gen = synth.e5a_iq if system == "5X" else synth.l5_iq
        self.iq = gen(fs, self.n, [self.sat], seed_offset=3)
        self.iq.setflags(write=False)
        self.delay, self.dop = float(start_sample), float(250 * round(doppler_hz / 250))
        ci, cq = primary_codes(system, prn)
        self.code, self.data_code = (cq, ci) if pilot else (ci, None)
        self.secondary = self.sat.sec_q if (system == "5X" and pilot) else None
        self.vl = int(round(fs / 1000))
        self.swap = SWAP[(system, pilot)]
        self.spb = SYMBOLS_PER_BIT[system]
        self.first = start_sample + self.vl  # fmod of a negative delta (:1822-1826): the second code start
        k0 = -int(-(fs - self.first) // self.vl)  # first call with (nitems_read - stamp) / (int)fs >= 1
        assert (k0 + 1) % 100 == 0
        self.sync_call = k0 + SYNC_LEN[(system, pilot)] - 1
        self.tag = "%s%s@%g" % (system, "pilot" if pilot else "data", fs)

    def conf(self, nch=1, item=gsdr.ITEM_GR_COMPLEX):
        c = _conf_sig(self.fs, SIGNAL[self.system], nch, self.pilot)
        c["item_type"] = item
        return c

    def restatement(self):
        """A started trk_restatement.Channel and its first sample."""
        import trk_restatement
        from oracle import trk
        ch = trk_restatement.Channel(self.conf()[0:1].view(trk.TRK_CONF_DTYPE), secondary_code=self.secondary)
        first = ch.start(self.code, self.delay, self.dop, 0, 0, prn=self.prn, data_code=self.data_code)
        return ch, first

    def transmitted(self, epochs):
        return synth.wideband_bit_signs(self.fs, self.n, self.sat, self.spb, epochs)


@functools.lru_cache(maxsize=None)
def case(system, pilot, fs=4.0e6):
    return Case(system, pilot, fs)


def data_component(recs, case_):
    """The valid outputs' d_P_data_accu rebuilt from prompt_i / prompt_q with the swap
    applied (prompt_i holds imag where d_interchange_iq is on), and of it the component
    that carries the data symbols: the PLL puts the tracked component on the real axis,
    so data tracking finds them in the real part and pilot tracking, whose data
    component is in quadrature, in the imaginary part.  For 5X that is prompt_i in both
    modes; for L5 the reference swaps the other way round (:242) and it is prompt_q."""
    out = np.nonzero(recs["flags"] & gsdr.TRK_F_VALID_OUTPUT)[0]
    pi, pq = recs["prompt_i"][out], recs["prompt_q"][out]
    re, im = (pq, pi) if case_.swap else (pi, pq)
    return out, (im if case_.pilot else re)


def check_locked_run(recs, case_):
    """One BIT_SYNC at the scenario's call, state 4 at the end, a valid output every
    symbols_per_bit calls from there, and the transmitted bit signs (all or all inverted)."""
    sync = np.nonzero(recs["flags"] & gsdr.TRK_F_BIT_SYNC)[0]
    assert list(sync) == [case_.sync_call], (case_.tag, sync)
    assert recs["state"][-1] == 4 and not np.any(recs["flags"] & gsdr.TRK_F_LOSS_OF_LOCK), case_.tag
    out, sym = data_component(recs, case_)
    assert len(out) >= 5 and out[0] == case_.sync_call + case_.spb and np.all(np.diff(out) == case_.spb), (case_.tag, out)
    # call k correlates code epoch k + 1: the output at call c closes the bit that holds epoch c + 1
    want = case_.transmitted(out + 1)
    got = np.sign(sym)
    assert np.all(got == want) or np.all(got == -want), (case_.tag, got, want)

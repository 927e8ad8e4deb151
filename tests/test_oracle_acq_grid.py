"""CPU pins of what the per-call dwell and moved-Doppler-grid GPU tests rest on
(tests/test_gpu_acq_dwell_calls.py, tests/test_gpu_acq_doppler_grid.py): the oracle's own
handling of doppler_center and doppler_bias (pcps_acquisition.cc:298-305: the carrier of
row d is float(bias + (-max + centre + step d)); :535 reports the Doppler without the
bias), oracle_dwell_sequence against _oracle_attempt, and the distance of every input
those tests use from a near tie, so that a seed cannot drift into one unnoticed."""
import numpy as np
import pytest

from oracle import pcps

import acq_checks
from acq_checks import (DWELL_CASES, DWELL_MARGIN, GRID_CASES, SET_DOPPLER_SIZES, _oracle_attempt, chain_args,
                        dwell_case, oracle_dwell_sequence, row_maxima_margin, size_case)

FS, N = 4000000, 4000


@pytest.mark.parametrize("mode", pcps.WIPE_MODES)
def test_center_moves_the_rows(mode):
    """Row d of the +-1000 / 250 Hz grid centred on 500 Hz is, bit for bit, row d + 4 of
    the +-1500 / 250 Hz grid centred on 0: the same integer Doppler, the same carrier."""
    a = pcps.doppler_wipeoffs(FS, N, 1000, 250, 8, doppler_center=500, mode=mode)
    b = pcps.doppler_wipeoffs(FS, N, 1500, 250, 12, doppler_center=0, mode=mode)
    for d in range(8):
        assert pcps.doppler_hz(d, 1000, 250, 500) == pcps.doppler_hz(d + 4, 1500, 250)
        assert a[d].tobytes() == b[d + 4].tobytes(), d
    # and a centre that is no multiple of the step moves every row off the old grid
    c = pcps.doppler_wipeoffs(FS, N, 1000, 250, 8, doppler_center=-375, mode=mode)
    assert [pcps.doppler_hz(d, 1000, 250, -375) for d in range(8)] == list(range(-1375, 625, 250))
    assert c[3].tobytes() == pcps.carrier(np.float32(-625), FS, N, mode).tobytes()


@pytest.mark.parametrize("mode", pcps.WIPE_MODES)
@pytest.mark.parametrize("bias", [562500, -1687500])
def test_bias_moves_the_carrier_only(bias, mode):
    """Row d with doppler_bias b is carrier(float32(b + doppler_hz(d))); doppler_hz, and so
    the reported Doppler of acquire(), does not carry the bias."""
    w = pcps.doppler_wipeoffs(FS, N, 1000, 250, 8, doppler_center=500, doppler_bias=bias, mode=mode)
    for d in range(8):
        f = np.float32(bias + pcps.doppler_hz(d, 1000, 250, 500))
        assert w[d].tobytes() == pcps.carrier(f, FS, N, mode).tobytes(), d
    if mode == "exact":
        case = size_case(N, 1000, 250, 500, bias)
        r = pcps.acquire(case.x, case.codes[0], case.fs, 1000, 250, pfa=0.01, doppler_center=500, doppler_bias=bias)
        assert r.doppler_hz == -1000 + 500 + 250 * r.index_doppler
        assert abs(r.doppler_hz - case.sats[0].doppler_hz) <= 125
        ti, di = pcps.max_to_input_power_statistic(case.grids[0])[:2]
        assert (r.index_time, r.index_doppler) == (ti, di)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("name", ["lds4000", "bt8000"])
def test_dwell_sequence_truncated_is_the_attempt(name, pfa):
    """oracle_dwell_sequence cut at the first crossing (else the last dwell) is
    _oracle_attempt's decision, grids included; thresholds chosen so that the PRNs stop
    at different dwells."""
    c = dwell_case(name)
    seq = c.seq(pfa)
    assert seq is c.seq(pfa)  # built once
    stats = sorted(float(s[0][4]) for s in seq)
    for thr in (0.5 * stats[0], 0.5 * (stats[1] + stats[2]), 2.0 * max(float(e[4]) for s in seq for e in s)):
        att = _oracle_attempt(c.chunks[:c.K], c.codes, pfa, c.D, c.dmax, c.dstep, c.bt, c.spc, thr, fs=c.fs)
        stops = set()
        for p, o in enumerate(att):
            k = next((k for k in range(c.K) if seq[p][k][4] > thr), c.K - 1)
            assert o[0] == k
            for got, want in zip(o[1:6], seq[p][k][:5]):
                assert got == want
            assert o[6].tobytes() == seq[p][k][5].tobytes()
            stops.add(k)
        if c.K > 1 and stats[0] < thr < stats[2]:
            assert len(stops) > 1
    # with a centre: the same sequence as the one built by hand from the moved wipe-offs
    if name == "lds4000" and pfa > 0:
        m = dwell_case("moved4000")
        assert m.center == 500
        wipe = pcps.doppler_wipeoffs(m.fs, m.N, m.dmax, m.dstep, m.D, 500)
        M0 = pcps.magnitude_grid(m.chunks[0], wipe, pcps.fft_code(m.codes[0], m.N, m.N))
        assert M0.tobytes() == m.seq(pfa)[0][0][5].tobytes()
        sq = oracle_dwell_sequence(m.chunks[:1], m.codes[:1], pfa, m.D, m.dmax, m.dstep, False, m.spc, fs=m.fs)
        assert sq[0][0][5].tobytes() != M0.tobytes()


@pytest.mark.parametrize("name", sorted(DWELL_CASES))
def test_dwell_inputs_are_far_from_a_near_tie(name):
    """Every visible PRN, at every dwell of both attempts: the two largest row maxima of the
    oracle's accumulated grid differ by more than 1e-3 relative, so the GPU has no excuse
    for another Doppler row; the visible PRNs are detected, the peak lands in the row of
    the satellite's Doppler."""
    c = dwell_case(name)
    worst = 1.0
    for first in (0, c.K):
        for pfa in (0.01, 0.0):
            seq = c.seq(pfa, first)
            for p in range(c.nvis):
                for k in range(c.K):
                    worst = min(worst, row_maxima_margin(seq[p][k][5]))
    print("near-tie margin", name, worst)
    assert worst > DWELL_MARGIN, (name, worst)


@pytest.mark.parametrize("name", ["bt8000", "bt12000"])
def test_bit_transition_peaks_sit_at_the_row_ends(name):
    """Satellite 0 peaks within samples_per_chip of the start of the N/2-entry row (the
    window wraps below zero, to N - ...), satellite 1 within samples_per_chip of its end
    (the window runs past the row while the wrap is at N)."""
    c = dwell_case(name)
    half = c.N // 2
    for first in (0, c.K):
        seq = c.seq(0.0, first)
        assert seq[0][0][0] < c.spc, seq[0][0][0]
        assert half > seq[1][0][0] >= half - c.spc, seq[1][0][0]
        assert c.spc <= seq[2][0][0] < half - c.spc


@pytest.mark.parametrize("key", sorted(GRID_CASES))
def test_grid_inputs_are_far_from_a_near_tie(key):
    """The one-block cases of the moved / biased grids: visible PRNs' row maxima apart by
    more than 1e-3, and the satellites' Dopplers inside the moved grid."""
    for args in GRID_CASES[key]:
        c = size_case(*args)
        for p in range(c.nvis):
            assert row_maxima_margin(c.grids[p]) > DWELL_MARGIN, (args, p)
            assert c.center - c.dmax < c.sats[p].doppler_hz < c.center + c.dmax, (args, p)


@pytest.mark.parametrize("N", sorted(SET_DOPPLER_SIZES))
def test_set_doppler_chain_inputs_are_far_from_a_near_tie(N):
    """The same for every step of the set_doppler chain; the PRNs do not change along it."""
    prns = None
    for step in ((1000, 250, 0),) + tuple(SET_DOPPLER_SIZES[N]):
        c = size_case(*chain_args(N, step))
        prns = c.prns if prns is None else prns
        assert (c.prns == prns).all()
        for p in range(c.nvis):
            assert row_maxima_margin(c.grids[p]) > DWELL_MARGIN, (N, step, p)


def test_float32_oracle_distance():
    """The reference arithmetic (complex64 FFTs) against the float64 oracle on the inputs
    of the dwell cases: the distance the GPU figures are read beside.  The accumulated
    grid's peak moves by less than RTOL / 2, so RTOL needs no widening for the per-call
    sums (the two summation orders of the one-shot and the per-call form included)."""
    c = dwell_case("lds4000")
    wipe = pcps.doppler_wipeoffs(c.fs, c.N, c.dmax, c.dstep, c.D)
    worst_grid = worst_peak = 0.0
    for p in range(c.nvis):
        acc32 = None
        for k in range(c.K):
            cf = pcps.fft_code(c.codes[p], c.N, c.N, dtype=np.complex64)
            M = pcps.magnitude_grid(c.chunks[k], wipe, cf, dtype=np.complex64)
            acc32 = M if acc32 is None else (acc32 + M).astype(np.float32)
            acc64 = c.seq(0.01)[p][k][5]
            worst_grid = max(worst_grid, float(np.abs(acc32.astype(np.float64) - acc64).max() / acc64.max()))
            worst_peak = max(worst_peak, abs(float(acc32.max()) - float(acc64.max())) / float(acc64.max()))
    print("float32 oracle vs float64: grid %.3g peak %.3g" % (worst_grid, worst_peak))
    assert worst_grid <= acq_checks.GRID_TOL
    assert worst_peak <= acq_checks.RTOL / 2

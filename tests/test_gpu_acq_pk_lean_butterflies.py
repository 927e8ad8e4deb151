"""Correlate variant 103 of N = 4000 (acq_pk.hip PkVariants): variant 101 -- PRN groups,
lane-order code rows, the prime-factor 32 x 125 plan of fft_pk.h -- with fewer instructions
in its butterflies (PkPfaPlan4000Lean): the 16-instruction 5-point transform DftLean<5> in
the first stage's radix 25 and in the last stage, whose outputs 1, 4 and 2, 3 reach the row
statistic two at a time, as a register pair of real parts and one of imaginary parts,
squared in packed instructions.

Other roundings than variant 101's, so, as for 101 in test_gpu_acq_pk_prime_factor.py: row
maxima against the float64 oracle within max(2 x variant 70's deviation on the same inputs,
12 * 2^-24) -- a bound from the reference variant, never from 103 --, the impulse sweep
through every output of the last stage against variant 70 under the same bound, and the
records (written by the argmax pass on the old plan) byte for byte against variant 70 on
inputs without a near-tie of Doppler rows.  Measured on MI355X: see
profiles/lean103/README.md.

Shapes, seeds and PRN counts are test_gpu_acq_pk_prime_factor.py's: 5 Doppler rows x 3
blocks, PRN counts around the group size of 16, seed offsets 72 (random data) and 80
(records: best and second-best row maxima 3.5e-3 apart at the least).
"""
import numpy as np
import pytest

import gsdr
from gsdr import synth

from acq_checks import PEAK_RATIO_THRESHOLD, _codes, _oracle_grids

pytestmark = pytest.mark.gpu

FS, N, DMAX, DSTEP, D, NBLOCKS = 4000000, 4000, 500, 250, 5, 3
REFERENCE, LEAN, PG = 70, 103, 16
COUNTS = (1, PG - 1, PG, PG + 1, 2 * PG + 3)
FLOOR = 12 * 2.0 ** -24
SEED_RANDOM, SEED_RECORDS = 72, 80

_inputs = {}


def _signal(seed):
    """(satellites, three blocks of IQ) of a seed, computed once."""
    if seed not in _inputs:
        sats = synth.random_constellation(6, seed_offset=seed, cn0_dbhz=50.0, max_doppler=DMAX - 100.0)
        x = synth.gps_l1_iq(FS, N * NBLOCKS, sats, seed_offset=seed)
        x.setflags(write=False)
        _inputs[seed] = (sats, x)
    return _inputs[seed]


def _prns(nprn, seed=SEED_RECORDS):
    """nprn PRN numbers, the visible ones first, then the rest of 1..32 (cyclically)."""
    vis = [s.prn for s in _signal(seed)[0]]
    rest = [p for p in range(1, 33) if p not in vis]
    return np.array([(vis + rest)[i % 32] for i in range(nprn)])


def _new(monkeypatch, variant, max_prns, pfa):
    monkeypatch.setenv("GSDR_ACQ_CORR_VARIANT", str(variant))
    acq = gsdr.Acquisition(FS, N, DMAX, DSTEP, pfa=pfa, max_prns=max_prns, max_blocks=NBLOCKS, num_doppler_bins=D)
    assert acq.fft_size == N and acq.num_doppler_bins == D
    if not pfa > 0:
        acq.set_threshold(PEAK_RATIO_THRESHOLD)
    return acq


def _handle(monkeypatch, variant, nprn, pfa, seed=SEED_RECORDS):
    acq = _new(monkeypatch, variant, nprn, pfa)
    prns = _prns(nprn, seed)
    acq.set_local_codes(_codes(prns, FS, N), prns)
    return acq


def _run(acq, seed=SEED_RECORDS):
    return acq.run(_signal(seed)[1], nblocks=NBLOCKS)


def _row_maxima(acq, x):
    """[NBLOCKS, D, nprn] float32 row maxima of the handle's correlate variant."""
    return np.stack([acq.dump_row_maxima(x[b * N:(b + 1) * N]) for b in range(NBLOCKS)])


_oracle = {}


def _oracle_maxima(seed):
    """[NBLOCKS, D, 35] row maxima of the oracle grids of a seed's signal, computed once
    (the PRN lists of the smaller counts are prefixes of the largest)."""
    if seed not in _oracle:
        x = _signal(seed)[1]
        codes = _codes(_prns(max(COUNTS), seed), FS, N)
        out = np.empty((NBLOCKS, D, max(COUNTS)))
        for b in range(NBLOCKS):
            grids = _oracle_grids(x[b * N:(b + 1) * N], codes, FS, DMAX, DSTEP, D)
            out[b] = np.stack([g.max(axis=1) for g in grids], axis=1)
        out.setflags(write=False)
        _oracle[seed] = out
    return _oracle[seed]


# ---------------------------------------------------------------- row maxima

_measured = []


def _bound(monkeypatch):
    """(bound, variant 70's and variant 103's largest relative deviation from the oracle's
    row maxima) over all blocks, rows and PRN counts of the seeded signal, measured once."""
    if not _measured:
        x = _signal(SEED_RANDOM)[1]
        ref = _oracle_maxima(SEED_RANDOM)
        dev = {REFERENCE: 0.0, LEAN: 0.0}
        for nprn in COUNTS:
            for variant in dev:
                got = _row_maxima(_handle(monkeypatch, variant, nprn, 0.01, SEED_RANDOM), x).astype(np.float64)
                assert got.shape == (NBLOCKS, D, nprn)
                dev[variant] = max(dev[variant], float(np.max(np.abs(got - ref[:, :, :nprn]) / ref[:, :, :nprn])))
        _measured.extend([max(2.0 * dev[REFERENCE], FLOOR), dev[REFERENCE], dev[LEAN]])
        print("row maxima against the oracle: variant %d %.3e, variant %d %.3e, bound %.3e"
              % (REFERENCE, dev[REFERENCE], LEAN, dev[LEAN], _measured[0]))
    return _measured


def _assert_rows_apart(monkeypatch, nprn):
    """The condition of the record tests, on the inputs: no near-tie of Doppler rows."""
    ref = np.sort(_oracle_maxima(SEED_RECORDS)[:, :, :nprn], axis=1)
    gap = (ref[:, -1] - ref[:, -2]) / ref[:, -1]
    assert gap.min() > 100.0 * _bound(monkeypatch)[0], ("inputs: near-tie of Doppler rows", gap.min())


def test_lean_random_data(monkeypatch):
    bound, dev70, dev103 = _bound(monkeypatch)
    assert dev103 <= bound, (dev103, dev70, bound)


def test_lean_every_output_path(monkeypatch):
    """IQ = a unit impulse at sample 0, so X = 1 in every Doppler row; slot p's code a real
    unit impulse at sample n_p, n_p sweeping 0 .. 3999 in 125 runs of 32 slots: each row's
    transform has one peak, and the peaks visit every output of the last stage once --
    both members of every pair, the two single outputs of a butterfly, and the partially
    filled second pass (lanes 128 to 143 of wave 2)."""
    bound = _bound(monkeypatch)[0]
    nprn = 32
    prns = np.arange(1, nprn + 1)
    x = np.zeros(N, np.complex64)
    x[0] = 1.0
    acqs = [_new(monkeypatch, v, nprn, 0.01) for v in (REFERENCE, LEAN)]
    worst = 0.0
    for run in range(N // nprn):
        codes = np.zeros((nprn, N), np.complex64)
        codes[np.arange(nprn), run * nprn + np.arange(nprn)] = 1.0
        got = []
        for acq in acqs:
            acq.set_local_codes(codes, prns)
            got.append(acq.dump_row_maxima(x).astype(np.float64))
        assert got[0].shape == (D, nprn) and got[0].min() > 0.5 * N * N, (run, got[0].min())
        dev = np.abs(got[1] - got[0]) / got[0]
        worst = max(worst, float(dev.max()))
        assert dev.max() <= bound, (run, np.argwhere(dev > bound)[:8], dev.max(), bound)
    print("every output path: largest relative deviation %.3e, bound %.3e" % (worst, bound))


# ---------------------------------------------------------------- records

_reference = {}


def _reference_bytes(monkeypatch, nprn, pfa):
    """Variant 70's result records of (nprn, pfa), computed once."""
    if (nprn, pfa) not in _reference:
        _reference[(nprn, pfa)] = _run(_handle(monkeypatch, REFERENCE, nprn, pfa)).tobytes()
    return _reference[(nprn, pfa)]


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("nprn", COUNTS)
def test_lean_records_equal_one_prn_per_workgroup(monkeypatch, nprn, pfa):
    _assert_rows_apart(monkeypatch, nprn)
    ref = _reference_bytes(monkeypatch, nprn, pfa)
    res = _run(_handle(monkeypatch, LEAN, nprn, pfa))
    assert res.shape == (NBLOCKS, nprn)
    assert res.tobytes() == ref


def test_lean_same_handle_twice(monkeypatch):
    nprn = 2 * PG + 3
    _assert_rows_apart(monkeypatch, nprn)
    acq = _handle(monkeypatch, LEAN, nprn, 0.01)
    first = _run(acq).tobytes()
    assert _run(acq).tobytes() == first
    assert first == _reference_bytes(monkeypatch, nprn, 0.01)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_lean_copy_follows_set_local_code(monkeypatch, pfa):
    """One slot's code replaced after a run: the lane-order row of that slot is the new
    code's, every other row is untouched -- the records of a fresh handle given the final
    codes.  Slot 2 holds a visible PRN before and an absent one after, and the last slot
    (the one-PRN group) gets a visible PRN in place of an absent one."""
    nprn = PG + 1
    _assert_rows_apart(monkeypatch, nprn)
    prns = _prns(nprn)
    final = prns.copy()
    final[2], final[nprn - 1] = prns[nprn - 1], prns[2]
    acq = _handle(monkeypatch, LEAN, nprn, pfa)
    before = _run(acq).tobytes()
    for slot in (2, nprn - 1):
        acq.set_local_code(slot, _codes(final[slot:slot + 1], FS, N)[0], int(final[slot]))
    got = _run(acq).tobytes()
    for variant in (LEAN, REFERENCE):
        fresh = _new(monkeypatch, variant, nprn, pfa)
        fresh.set_local_codes(_codes(final, FS, N), final)
        assert got == _run(fresh).tobytes(), variant
    assert got != before


def test_lean_copy_follows_second_set_local_codes(monkeypatch):
    """A second set_local_codes (other PRNs in every slot, and fewer of them) replaces
    every lane-order row it loads."""
    nprn = 2 * PG + 3
    _assert_rows_apart(monkeypatch, nprn)
    acq = _handle(monkeypatch, LEAN, nprn, 0.01)
    _run(acq)
    second = _prns(nprn)[::-1][:PG + 1].copy()
    acq.set_local_codes(_codes(second, FS, N), second)
    got = _run(acq)
    assert got.shape == (NBLOCKS, PG + 1)
    fresh = _new(monkeypatch, REFERENCE, nprn, 0.01)
    fresh.set_local_codes(_codes(second, FS, N), second)
    assert got.tobytes() == _run(fresh).tobytes()


@pytest.mark.parametrize("active", [1, PG - 1, PG + 1])
def test_lean_fewer_active_prns(monkeypatch, active):
    nprn = 2 * PG + 3
    _assert_rows_apart(monkeypatch, nprn)
    acq = _handle(monkeypatch, LEAN, nprn, 0.01)
    ref = _handle(monkeypatch, REFERENCE, nprn, 0.01)
    acq.set_active_prns(active)
    ref.set_active_prns(active)
    got = _run(acq)
    assert got.shape == (NBLOCKS, active)
    assert got.tobytes() == _run(ref).tobytes()


def test_lean_step_two(monkeypatch):
    """run_step_two launches on one-PRN views: each needs its own code row, in the
    variant's lane order, whichever kernel the view reaches."""
    nprn, nbins2, step2 = PG + 1, 5, 100.0
    _assert_rows_apart(monkeypatch, nprn)
    x = _signal(SEED_RECORDS)[1]
    out = []
    for variant in (LEAN, REFERENCE):
        acq = _handle(monkeypatch, variant, nprn, 0.01)
        acq.set_step_two(nbins2, step2)
        first = acq.run(x[:N])[0]
        sel = np.nonzero(first["positive"])[0]
        assert len(sel) >= 2, first
        # the visible PRNs are in the first slots; the last slot is the one-PRN group's
        sel = np.concatenate([sel, [nprn - 1]])
        fine = acq.run_step_two(x[N:2 * N], sel, first["doppler_hz"][sel].astype(np.float32),
            first["input_power"][sel], stamp=N)
        again = acq.run(x[:N])[0]
        assert again.tobytes() == first.tobytes()
        out.append((first.tobytes(), fine.tobytes()))
    assert out[0] == out[1]

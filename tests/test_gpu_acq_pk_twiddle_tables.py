"""Correlate variant 99 of N = 4000 (acq_pk.hip PkVariants: variant 98 with the inter-stage
twiddles read from two tables in the workgroup's LDS -- the middle stage's powers w^r and a
copy of the last stage's roots, built once per workgroup behind the FFT buffer and the
statistics scratch) against variant 70, one PRN per workgroup, twiddles from global memory.

The factors have the same bits wherever they are fetched from, so the row maxima and with
them every byte of the result records are equal.  A wrong table slot, a table read before
the barrier that publishes it, or a code-row copy that lands on a table changes a row
maximum and shows here.

Shape, as test_gpu_acq_pk_lane_order.py: N = 4000 (the plan fixes it), 5 Doppler rows x 3
blocks = 15 (b, d) rows -- 8 in the XCD-balanced part of the workgroup mapping, 7 in its
linear tail -- and PRN counts around the group size of 16: a one-PRN workgroup builds its
tables and uses them once, a 16-PRN workgroup reuses them 15 times.
"""
import numpy as np
import pytest

import gsdr
from gsdr import synth

from acq_checks import PEAK_RATIO_THRESHOLD, _check_result, _codes, _oracle_grids

pytestmark = pytest.mark.gpu

FS, N, DMAX, DSTEP, D, NBLOCKS = 4000000, 4000, 500, 250, 5, 3
REFERENCE, TABLES, PG = 70, 99, 16
COUNTS = (1, PG - 1, PG, PG + 1, 2 * PG + 3)

_input = []


def _signal():
    """(satellites, three blocks of IQ), computed once."""
    if not _input:
        sats = synth.random_constellation(6, seed_offset=72, cn0_dbhz=50.0, max_doppler=DMAX - 100.0)
        x = synth.gps_l1_iq(FS, N * NBLOCKS, sats, seed_offset=72)
        x.setflags(write=False)
        _input.extend([sats, x])
    return _input


def _prns(nprn):
    """nprn PRN numbers, the visible ones first, then the rest of 1..32 (cyclically)."""
    vis = [s.prn for s in _signal()[0]]
    rest = [p for p in range(1, 33) if p not in vis]
    return np.array([(vis + rest)[i % 32] for i in range(nprn)])


def _new(monkeypatch, variant, max_prns, pfa):
    monkeypatch.setenv("GSDR_ACQ_CORR_VARIANT", str(variant))
    acq = gsdr.Acquisition(FS, N, DMAX, DSTEP, pfa=pfa, max_prns=max_prns, max_blocks=NBLOCKS, num_doppler_bins=D)
    assert acq.fft_size == N and acq.num_doppler_bins == D
    if not pfa > 0:
        acq.set_threshold(PEAK_RATIO_THRESHOLD)
    return acq


def _handle(monkeypatch, variant, nprn, pfa):
    acq = _new(monkeypatch, variant, nprn, pfa)
    prns = _prns(nprn)
    acq.set_local_codes(_codes(prns, FS, N), prns)
    return acq


def _run(acq):
    return acq.run(_signal()[1], nblocks=NBLOCKS)


_reference = {}


def _reference_bytes(monkeypatch, nprn, pfa):
    """Variant 70's result records of (nprn, pfa), computed once."""
    if (nprn, pfa) not in _reference:
        _reference[(nprn, pfa)] = _run(_handle(monkeypatch, REFERENCE, nprn, pfa)).tobytes()
    return _reference[(nprn, pfa)]


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("nprn", COUNTS)
def test_twiddle_tables_equal_one_prn_per_workgroup(monkeypatch, nprn, pfa):
    ref = _reference_bytes(monkeypatch, nprn, pfa)
    res = _run(_handle(monkeypatch, TABLES, nprn, pfa))
    assert res.shape == (NBLOCKS, nprn)
    assert res.tobytes() == ref


def test_twiddle_tables_same_handle_twice(monkeypatch):
    """PG + 1 PRNs: per (b, d) row one workgroup of 16 PRNs and one of a single PRN."""
    nprn = PG + 1
    acq = _handle(monkeypatch, TABLES, nprn, 0.01)
    first = _run(acq).tobytes()
    assert _run(acq).tobytes() == first
    assert first == _reference_bytes(monkeypatch, nprn, 0.01)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_twiddle_tables_after_set_local_code(monkeypatch, pfa):
    """One slot's code replaced after a run (slot 2: a visible PRN before, an absent one
    after; the last slot, the one-PRN group: the reverse): the records of a fresh
    variant-70 handle given the final codes."""
    nprn = PG + 1
    prns = _prns(nprn)
    final = prns.copy()
    final[2], final[nprn - 1] = prns[nprn - 1], prns[2]
    acq = _handle(monkeypatch, TABLES, nprn, pfa)
    before = _run(acq).tobytes()
    for slot in (2, nprn - 1):
        acq.set_local_code(slot, _codes(final[slot:slot + 1], FS, N)[0], int(final[slot]))
    got = _run(acq).tobytes()
    fresh = _new(monkeypatch, REFERENCE, nprn, pfa)
    fresh.set_local_codes(_codes(final, FS, N), final)
    assert got == _run(fresh).tobytes()
    assert got != before


def test_twiddle_tables_after_second_set_local_codes(monkeypatch):
    """A second set_local_codes: other PRNs in every slot, and fewer of them."""
    nprn = 2 * PG + 3
    acq = _handle(monkeypatch, TABLES, nprn, 0.01)
    _run(acq)
    second = _prns(nprn)[::-1][:PG + 1].copy()
    acq.set_local_codes(_codes(second, FS, N), second)
    got = _run(acq)
    assert got.shape == (NBLOCKS, PG + 1)
    fresh = _new(monkeypatch, REFERENCE, nprn, 0.01)
    fresh.set_local_codes(_codes(second, FS, N), second)
    assert got.tobytes() == _run(fresh).tobytes()


@pytest.mark.parametrize("active", [1, PG - 1, PG + 1])
def test_twiddle_tables_fewer_active_prns(monkeypatch, active):
    nprn = 2 * PG + 3
    acq = _handle(monkeypatch, TABLES, nprn, 0.01)
    ref = _handle(monkeypatch, REFERENCE, nprn, 0.01)
    acq.set_active_prns(active)
    ref.set_active_prns(active)
    got = _run(acq)
    assert got.shape == (NBLOCKS, active)
    assert got.tobytes() == _run(ref).tobytes()


def test_twiddle_tables_step_two(monkeypatch):
    """run_step_two launches on one-PRN views: every workgroup builds its tables for a
    single transform."""
    nprn, nbins2, step2 = PG + 1, 5, 100.0
    x = _signal()[1]
    out = []
    for variant in (TABLES, REFERENCE):
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


def test_twiddle_tables_match_oracle(monkeypatch):
    """11 PRNs, 6 of them visible, against the oracle grids of every block, at
    test_gpu_acq_pk_lane_order.py's bars."""
    nprn, pfa = 11, 0.01
    prns = _prns(nprn)
    codes = _codes(prns, FS, N)
    x = _signal()[1]
    res = _run(_handle(monkeypatch, TABLES, nprn, pfa))
    for b in range(NBLOCKS):
        grids = _oracle_grids(x[b * N:(b + 1) * N], codes, FS, DMAX, DSTEP, D)
        exact = [_check_result(res[b, p], grids[p], pfa, 4, FS, DMAX, DSTEP, 4000.0) for p in range(nprn)]
        assert sum(exact) >= nprn - 1, (b, exact)
        assert [int(r["prn"]) for r in res[b]] == list(prns)

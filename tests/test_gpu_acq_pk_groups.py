"""The PRN-group correlate variants of N = 4000 (acq_pk.hip PkVariants, code source
kCodeLds: X resident for a group of PG PRNs, each next code row copied into the
drained FFT buffer by buffer_load ... lds) against variant 70, one PRN per workgroup.

The arithmetic of a transform is the same in both, so the row maxima and with them
every byte of the result records are equal.  A stale or half-landed code row, a copy
that runs into the statistics scratch behind the buffer, or a leftover of the previous
group changes a row maximum and shows here.

Shape: N = 4000 (the plan fixes it), 5 Doppler rows x 3 blocks = 15 (b, d) rows -- 8
in the XCD-balanced part of the workgroup mapping, 7 in its linear tail -- and PRN
counts around the group size: a group shorter than PG, an exact group, a last group
of one PRN, and two groups and a short third (the guard on the next-row copy).
"""
import numpy as np
import pytest

import gsdr
from gsdr import synth

from acq_checks import PEAK_RATIO_THRESHOLD, _check_result, _codes, _oracle_grids

pytestmark = pytest.mark.gpu

FS, N, DMAX, DSTEP, D, NBLOCKS = 4000000, 4000, 500, 250, 5, 3
REFERENCE = 70
GROUPED = {97: 16}  # variant id -> PRNs per workgroup
CASES = [(v, n) for v, pg in GROUPED.items() for n in (1, pg - 1, pg, pg + 1, 2 * pg + 3)]

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


def _handle(monkeypatch, variant, nprn, pfa):
    monkeypatch.setenv("GSDR_ACQ_CORR_VARIANT", str(variant))
    acq = gsdr.Acquisition(FS, N, DMAX, DSTEP, pfa=pfa, max_prns=nprn, max_blocks=NBLOCKS, num_doppler_bins=D)
    assert acq.fft_size == N and acq.num_doppler_bins == D
    prns = _prns(nprn)
    acq.set_local_codes(_codes(prns, FS, N), prns)
    if not pfa > 0:
        acq.set_threshold(PEAK_RATIO_THRESHOLD)
    return acq


_reference = {}


def _reference_bytes(monkeypatch, nprn, pfa):
    """Variant 70's result records of (nprn, pfa), computed once."""
    if (nprn, pfa) not in _reference:
        _reference[(nprn, pfa)] = _handle(monkeypatch, REFERENCE, nprn, pfa).run(_signal()[1], nblocks=NBLOCKS).tobytes()
    return _reference[(nprn, pfa)]


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("variant,nprn", CASES)
def test_grouped_variant_equals_one_prn_per_workgroup(monkeypatch, variant, nprn, pfa):
    ref = _reference_bytes(monkeypatch, nprn, pfa)
    res = _handle(monkeypatch, variant, nprn, pfa).run(_signal()[1], nblocks=NBLOCKS)
    assert res.shape == (NBLOCKS, nprn)
    assert res.tobytes() == ref


@pytest.mark.parametrize("variant", sorted(GROUPED))
def test_grouped_variant_same_handle_twice(monkeypatch, variant):
    nprn = 2 * GROUPED[variant] + 3
    acq = _handle(monkeypatch, variant, nprn, 0.01)
    first = acq.run(_signal()[1], nblocks=NBLOCKS).tobytes()
    assert acq.run(_signal()[1], nblocks=NBLOCKS).tobytes() == first
    assert first == _reference_bytes(monkeypatch, nprn, 0.01)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("variant", sorted(GROUPED))
def test_grouped_variant_matches_oracle(monkeypatch, variant, pfa):
    """11 PRNs, 6 of them visible, against the oracle grids of every block."""
    nprn = 11
    prns = _prns(nprn)
    codes = _codes(prns, FS, N)
    x = _signal()[1]
    res = _handle(monkeypatch, variant, nprn, pfa).run(x, nblocks=NBLOCKS)
    for b in range(NBLOCKS):
        grids = _oracle_grids(x[b * N:(b + 1) * N], codes, FS, DMAX, DSTEP, D)
        exact = [_check_result(res[b, p], grids[p], pfa, 4, FS, DMAX, DSTEP, 4000.0) for p in range(nprn)]
        assert sum(exact) >= nprn - 1, (b, exact)
        assert [int(r["prn"]) for r in res[b]] == list(prns)

"""doppler_center, doppler_bias and gsdr_acq_set_doppler against the float64 oracle.

The host block calls gsdr_acq_set_doppler on every acquisition start, and it is the only
way an assisted centre reaches a live engine; the call re-derives the forward-spectrum
reuse layout (grid_xmap: q stored spectra, shift p).  The reference adds the bias to the
carrier only (pcps_acquisition.cc:302-303), not to the reported Doppler (:535, :572).

Every case: the dumped forward spectra, the dumped grid of a visible PRN and the records
of both statistics (acq_checks.check_size), on the reuse layout and on the plain layout
reached through the generic carrier model and through an incommensurate step.  Inputs:
acq_checks.GRID_CASES / SET_DOPPLER_SIZES, their near-tie margins pinned on the CPU."""
import numpy as np
import pytest

import gsdr
from oracle import pcps

from acq_checks import (GRID_BIASES, GRID_CENTERS, GRID_LAYOUTS, SET_DOPPLER_SIZES, SPECTRUM_TOL, chain_args,
                        check_records, check_size, dwell_case, grid_args, make_acq, size_case)

pytestmark = pytest.mark.gpu

PFAS = [0.01, 0.0]


def _on_grid(res, case):
    """doppler_hz is -max + centre + step d exactly: the centre in, the bias out."""
    for r in res:
        assert r["doppler_hz"] == -case.dmax + case.center + case.dstep * int(r["doppler_index"])


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("center", GRID_CENTERS)
@pytest.mark.parametrize("layout", sorted(GRID_LAYOUTS))
def test_center_at_create(layout, center, pfa):
    """doppler_center in the configuration: a multiple of the step, one that is none, and
    one that puts every row above zero; the satellites sit inside the moved grid."""
    case = size_case(*grid_args(layout, center))
    acq = make_acq(case, pfa)
    assert acq.spectrum_reuse == GRID_LAYOUTS[layout][3]
    res = check_size(acq, case, pfa, "center_%s_%d" % (layout, center))
    _on_grid(res, case)
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("bias,center", GRID_BIASES)
@pytest.mark.parametrize("layout", sorted(GRID_LAYOUTS))
def test_bias(layout, bias, center, pfa):
    """GLONASS L1 channels +1 and -3: the block carries the channel offset, the wipe-off
    rows are float(bias + Doppler), the reported Doppler is the row's without the bias."""
    case = size_case(*grid_args(layout, center, bias))
    acq = make_acq(case, pfa)
    assert acq.spectrum_reuse == GRID_LAYOUTS[layout][3]
    res = check_size(acq, case, pfa, "bias_%s_%d_%d" % (layout, bias, center))
    _on_grid(res, case)
    for p in range(case.nvis):
        assert abs(int(res[p]["doppler_hz"]) - case.sats[p].doppler_hz) < case.dmax
    acq.close()


def _same_as_fresh(acq, fresh, case, pfa, tag):
    """A live handle after set_doppler against a handle created with that configuration:
    layout, threshold, the records and spectra byte for byte, the narrow second step; and
    the live handle against the oracle."""
    assert acq.spectrum_reuse == fresh.spectrum_reuse, tag
    assert acq.threshold == fresh.threshold
    res = acq.run(case.x)[0]
    assert res.tobytes() == fresh.run(case.x)[0].tobytes(), tag
    assert acq.dump_spectra(case.x).tobytes() == fresh.dump_spectra(case.x).tobytes(), tag
    res = check_size(acq, case, pfa, tag)  # spectra, grid and records (the CFAR threshold too) against the oracle
    _on_grid(res, case)
    sel = np.arange(case.nvis)
    fine = []
    for h in (acq, fresh):
        h.set_step_two(4, 125.0)
        fine.append(h.run_step_two(case.x, sel, res["doppler_hz"][sel].astype(np.float32), res["input_power"][sel],
                                   stamp=77))
    assert fine[0].tobytes() == fine[1].tobytes(), tag
    assert (fine[0]["prn"] == case.prns[sel]).all()
    return res


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("N", sorted(SET_DOPPLER_SIZES))
def test_set_doppler_on_a_live_handle(N, pfa):
    """The centre alone, the step with the bin count kept (reuse q = 4 -> 2), the plain
    layout and back, on the N = 4000 packed-variant handle, an N = 6000 runtime-plan
    handle and the N = 25000 split handle; the codes are set once, before the first call."""
    case0 = size_case(*chain_args(N, (1000, 250, 0)))
    acq = make_acq(case0, pfa)
    plan = acq.plan
    if N == 25000:
        assert plan["split"] != 0, plan
    elif N == 6000:
        assert plan["variant"] in (10, 11, 12) and plan["split"] == 0, plan
    else:
        assert 1 <= plan["variant"] <= 4 and acq.dump_row_maxima(case0.x).shape == (case0.D, 4), plan
    assert acq.spectrum_reuse == (4, 1)
    prns0, codes0 = case0.prns.copy(), case0.codes.tobytes()
    reuse = {250: (4, 1), 500: (2, 1), 300: (8, 0)}
    for step in SET_DOPPLER_SIZES[N]:
        dmax, dstep, center = step
        case = size_case(*chain_args(N, step))
        assert (case.prns == prns0).all() and case.codes.tobytes() == codes0  # set once, at create
        acq.set_doppler(dmax, dstep, center)
        assert acq.spectrum_reuse == reuse[dstep], step
        assert acq.num_doppler_bins == case.D
        fresh = make_acq(case, pfa)
        assert fresh.plan == plan
        _same_as_fresh(acq, fresh, case, pfa, "set_doppler_%d_%d_%d_%d" % ((N,) + step))
        fresh.close()
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_set_doppler_refusals(pfa):
    """A call that would change the number of Doppler bins is unsupported, a zero step an
    argument error; the handle is as before.  With an explicit num_doppler_bins the bin
    count is the caller's and the check does not apply."""
    case = size_case(*grid_args("reuse", 500))
    acq = make_acq(case, pfa)
    before = acq.run(case.x)[0]
    X = acq.dump_spectra(case.x)
    for args, code in (((1000, 125, 500), gsdr.GSDR_E_UNSUPPORTED), ((1000, 0, 500), gsdr.GSDR_E_ARG),
                       ((2000, 250, 500), gsdr.GSDR_E_UNSUPPORTED)):
        with pytest.raises(gsdr.GsdrError) as e:
            acq.set_doppler(*args)
        assert e.value.code == code, args
        assert acq.spectrum_reuse == (4, 1)
        assert acq.run(case.x)[0].tobytes() == before.tobytes(), args
        assert acq.dump_spectra(case.x).tobytes() == X.tobytes(), args
    check_records(before, acq, case, pfa)
    acq.close()
    # explicit bin count: 8 rows of 125 Hz from -1000 + 500
    kw = dict(pfa=pfa, max_prns=len(case.prns), num_doppler_bins=8)
    live = gsdr.Acquisition(case.fs, case.N, 1000, 250, **kw)
    fresh = gsdr.Acquisition(case.fs, case.N, 1000, 125, doppler_center=500, **kw)
    for h in (live, fresh):
        h.set_local_codes(case.codes, case.prns)
    live.set_doppler(1000, 125, 500)
    for h in (live, fresh):
        if pfa > 0:  # the CFAR threshold follows the bin count, which the call kept
            assert abs(h.threshold - pcps.threshold(pfa, case.N, 8)) <= 1e-6 * h.threshold
        else:
            h.set_threshold(2.5)
    assert live.num_doppler_bins == fresh.num_doppler_bins == 8
    assert live.spectrum_reuse == fresh.spectrum_reuse
    res = live.run(case.x)[0]
    assert res.tobytes() == fresh.run(case.x)[0].tobytes()
    assert live.dump_spectra(case.x).tobytes() == fresh.dump_spectra(case.x).tobytes()
    for r in res:
        assert r["doppler_hz"] == -1000 + 500 + 125 * int(r["doppler_index"])
    wipe = pcps.doppler_wipeoffs(case.fs, case.N, 1000, 125, 8, 500)
    ref = np.fft.fft(case.x.astype(np.complex128)[None, :] * wipe.astype(np.complex128), axis=1)
    assert np.abs(live.dump_spectra(case.x) - ref).max() / np.abs(ref).max() < SPECTRUM_TOL
    for h in (live, fresh):
        h.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_dwell_calls_on_a_moved_grid(pfa):
    """The host block's call order: create, set_doppler (init), run_dwell x K -- the
    centre set after create and again between two attempts, against the oracle's dwell
    sequence on the moved grid."""
    c = dwell_case("moved4000")
    assert c.center == 500
    acq = c.make(pfa, center=0)
    acq.set_doppler(c.dmax, c.dstep, c.center)
    for first in (0, c.K):
        for k in range(c.K):
            recs = acq.run_dwell(c.chunks[first + k], k, 900 - 7 * k)
            c.check(recs, pfa, k, 900 - 7 * k, first)
        acq.set_doppler(c.dmax, c.dstep, 0)
        wrong = acq.run_dwell(c.chunks[0], 0, 1)
        assert (wrong["doppler_hz"] == -c.dmax + c.dstep * wrong["doppler_index"].astype(np.int64)).all()
        acq.set_doppler(c.dmax, c.dstep, c.center)
    acq.close()

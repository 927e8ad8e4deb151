"""The per-call dwell of the C ABI (gsdr_acq_run_dwell: acq_dwell_grid_kernel, launch_dwell,
acq_grid_second_peak_kernel) against the float64 oracle.

pcps_acquisition_mi355x::acquisition_core calls it once per block whenever max_dwells > 1:
dwell 0 writes the device grid of the attempt, later dwells add into it, and every call
reports the statistic of the grid accumulated so far with dwell + 1 as the CFAR divisor
(pcps_acquisition.cc:637-696).  tests/test_gpu_acq_dwells.py covers the one-shot form
(gsdr_acq_run with max_dwells), which sums in other kernels.

Inputs and oracle sequences: acq_checks.DWELL_CASES, built once per case; their distance
from a near tie is pinned on the CPU (tests/test_oracle_acq_grid.py)."""
import json

import numpy as np
import pytest

import gsdr
from gsdr import synth

from acq_checks import RTOL, check_dwell_record, dwell_case, oracle_dwell_sequence

pytestmark = pytest.mark.gpu

PFAS = [0.01, 0.0]
# distinct, neither increasing nor a multiple of the block: no stamp follows from the dwell index
STAMPS = (1000003, 17, 5000000011)


def _static(p):
    return 1 <= p["variant"] <= 4 and p["r1"] == 0 and p["split"] == 0


PLANS = {
    "lds4000": _static,                                                                  # compile-time LDS plan
    "runtime6000": lambda p: (p["variant"], p["nthreads"], p["split"]) == (11, 512, 0),  # runtime LDS plan
    "four40000": lambda p: (p["variant"], p["split"]) == (20, 0),                        # generic four-step
    "packed32000": lambda p: 24 <= p["variant"] <= 27 and p["split"] == 0,               # packed four-step
    "bt8000": _static,
    "bt12000": lambda p: (p["variant"], p["nthreads"], p["split"]) == (12, 1024, 0),
}


def _handle(name, pfa, **kw):
    c = dwell_case(name)
    acq = c.make(pfa, **kw)
    assert PLANS[name](acq.plan), acq.plan
    return c, acq


def _sequence(acq, c, first=0, dwells=None):
    """run_dwell over chunks first .. of one attempt -> the records of every call."""
    return [acq.run_dwell(c.chunks[first + k], k, STAMPS[k]) for k in range(c.K if dwells is None else dwells)]


def _log(tag, name, pfa, worst):
    print("parity acq", json.dumps({"tag": tag, "case": name, "pfa": pfa, **{k: float("%.3g" % v)
                                                                              for k, v in worst.items()}}))


def _distances(recs, seq, pfa, worst):
    """The measured GPU-versus-oracle distances of one call's records, kept as the worst."""
    for p, r in enumerate(recs):
        ti, di, peak, aux, stat, acc = seq[p]
        if (r["doppler_index"], r["code_phase"]) != (di, ti):
            continue
        worst["peak"] = max(worst["peak"], abs(float(r["peak"]) - float(peak)) / float(peak))
        worst["stat"] = max(worst["stat"], abs(float(r["test_statistic"]) - float(stat)) / float(stat))
        g = float(r["input_power"] if pfa > 0 else r["second_peak"])
        worst["aux"] = max(worst["aux"], abs(g - float(aux)) / float(aux))


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("name", ["lds4000", "runtime6000", "four40000", "packed32000"])
def test_sequence_matches_oracle(name, pfa):
    """After every run_dwell(x_k, k, stamp_k) each record is the oracle's of the grid
    accumulated over blocks 0..k: cell, peak, input power (divisor k + 1) or second peak,
    statistic, decision, num_dwells = k + 1, the Doppler of the cell and the stamp of that
    call.  4 active slots of 6; two attempts, so dwell 0 also restarts a used grid."""
    c, acq = _handle(name, pfa)
    worst = {"peak": 0.0, "stat": 0.0, "aux": 0.0}
    near = 0
    for first in (0, c.K):
        for k in range(c.K):
            recs = acq.run_dwell(c.chunks[first + k], k, STAMPS[k])
            assert len(recs) == len(c.prns)
            _distances(recs, [s[k] for s in c.seq(pfa, first)], pfa, worst)
            exact = c.check(recs, pfa, k, STAMPS[k], first)
            near = max(near, len(exact) - sum(exact))
    _log("dwell_calls", name, pfa, worst)
    assert near <= 1  # the absent PRN alone may sit on a near tie
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("name", ["lds4000", "runtime6000", "four40000", "packed32000"])
def test_agrees_with_the_one_shot_form(name, pfa):
    """gsdr_acq_run over the K blocks decides per PRN at its dwell n (num_dwells); the
    per-call record of dwell n - 1 on the same handle names the same cell (or both sit on
    an oracle near tie) and peak, statistic and input power / second peak agree within
    RTOL of the oracle's value.  The two forms sum in different kernels (the accumulator
    row pool against the kept grid), but both add block k to the float32 sum of blocks
    0..k-1 in the same order: on every case here the three values are bit-identical, and
    that is asserted."""
    c, acq = _handle(name, pfa)
    percall = _sequence(acq, c)
    one = acq.run(c.x[:c.K * c.N], stamp0=STAMPS[0])[0]
    thr = c.threshold(pfa)
    seq = c.seq(pfa)
    worst = {"peak": 0.0, "stat": 0.0, "aux": 0.0}
    aux_f = "input_power" if pfa > 0 else "second_peak"
    for p in range(len(c.prns)):
        n = int(one[p]["num_dwells"])
        want = next((k for k in range(c.K) if seq[p][k][4] > thr), c.K - 1) + 1
        if all(abs(seq[p][k][4] - thr) > 1e-3 * thr for k in range(c.K)):
            assert n == want, (p, n, want)
        assert 1 <= n <= c.K
        assert one[p]["samplestamp"] == STAMPS[0] + (n - 1) * c.N
        r = percall[n - 1][p]
        ti, di, peak, aux, stat, acc = seq[p][n - 1]
        if (one[p]["doppler_index"], one[p]["code_phase"]) != (r["doppler_index"], r["code_phase"]):
            assert p >= c.nvis, p
            for q in (one[p], r):
                assert abs(acc[q["doppler_index"], q["code_phase"]] - peak) <= RTOL * peak
            continue
        for f, ref in (("peak", peak), ("test_statistic", stat), (aux_f, aux)):
            d = abs(float(one[p][f]) - float(r[f])) / float(ref)
            key = {"peak": "peak", "test_statistic": "stat"}.get(f, "aux")
            worst[key] = max(worst[key], d)
            assert one[p][f] == r[f], (p, f, one[p][f], r[f])
        assert one[p]["positive"] == r["positive"] or abs(stat - thr) <= 1e-3 * thr
    _log("dwell_calls_vs_one_shot", name, pfa, worst)
    assert max(worst.values()) <= RTOL, worst
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("name", ["lds4000", "four40000"])
def test_dwell_zero_restarts_the_grid(name, pfa):
    """Dwell 0 overwrites the kept grid: after dwells 0 and 1 of attempt A, and again after
    a completed attempt, dwell 0 and dwell 1 of another input give the bytes of a fresh
    handle."""
    c, acq = _handle(name, pfa)
    _, fresh = _handle(name, pfa)
    ref_b = _sequence(fresh, c, first=c.K)
    _sequence(acq, c, first=0, dwells=2)                 # A abandoned after two dwells
    got_b = _sequence(acq, c, first=c.K)                 # B, completed
    for k in range(c.K):
        assert got_b[k].tobytes() == ref_b[k].tobytes(), k
        c.check(got_b[k], pfa, k, STAMPS[k], c.K)
    fresh.close()
    _, fresh = _handle(name, pfa)
    ref_a = _sequence(fresh, c, first=0, dwells=2)
    got_a = _sequence(acq, c, first=0, dwells=2)         # A again, after the completed B
    for k in range(2):
        assert got_a[k].tobytes() == ref_a[k].tobytes(), k
        c.check(got_a[k], pfa, k, STAMPS[k], 0)
    assert got_a[0].tobytes() != got_b[0].tobytes()
    for h in (acq, fresh):
        h.close()


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("name", ["lds4000", "runtime6000"])
def test_other_calls_leave_the_kept_grid(name, pfa):
    """dump_grid, dump_spectra and a one-shot run on other blocks between dwell 0 and
    dwell 1 (the host block dumps this way) leave the later dwells byte-identical; with
    the active PRN count lowered between attempts the next attempt is a 2-slot handle's."""
    c, acq = _handle(name, pfa)
    _, fresh = _handle(name, pfa)
    ref = _sequence(fresh, c)
    other = c.x[c.K * c.N:2 * c.K * c.N]
    r0 = acq.run_dwell(c.chunks[0], 0, STAMPS[0])
    assert r0.tobytes() == ref[0].tobytes()
    g = acq.dump_grid(c.chunks[c.K], 1)
    X = acq.dump_spectra(c.chunks[c.K + 1])
    assert g.shape == (c.D, c.N) and X.shape == (c.D, c.N)
    one = acq.run(other, stamp0=5)[0]
    assert len(one) == len(c.prns)
    for k in range(1, c.K):
        r = acq.run_dwell(c.chunks[k], k, STAMPS[k])
        assert r.tobytes() == ref[k].tobytes(), k
        c.check(r, pfa, k, STAMPS[k])
    fresh.close()
    acq.set_active_prns(2)
    _, two = _handle(name, pfa, nprn=2)
    for k in range(c.K):
        r = acq.run_dwell(c.chunks[c.K + k], k, STAMPS[k])
        r2 = two.run_dwell(c.chunks[c.K + k], k, STAMPS[k])
        assert len(r) == 2 and r.tobytes() == r2.tobytes(), k
        c.check(r, pfa, k, STAMPS[k], c.K)
    for h in (acq, two):
        h.close()


def _same_cell_or_tie(a, b, o, visible):
    ti, di, peak, aux, stat, acc = o
    if (a["doppler_index"], a["code_phase"]) == (b["doppler_index"], b["code_phase"]):
        return
    assert not visible
    for q in (a, b):
        assert abs(acc[q["doppler_index"], q["code_phase"]] - peak) <= RTOL * peak


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("name", ["lds4000", "split25000"])
def test_single_dwell_handles(name, pfa):
    """run_dwell(x, 0) on a max_dwells = 1 handle -- N = 4000 with its packed correlate
    variant, N = 25000 on the split correlate: the dwell kernel runs on the handle's plain
    FFT plan beside them; the record is the oracle's one-dwell record and names run(x)'s
    cell."""
    c = dwell_case(name)
    acq = c.make(pfa, max_dwells=1)
    if name == "split25000":
        assert acq.plan["split"] != 0, acq.plan
    else:
        assert acq.dump_row_maxima(c.chunks[0]).shape == (c.D, len(c.prns))  # a packed correlate variant
    for first in (0, 1):
        x = c.chunks[first]
        recs = acq.run_dwell(x, 0, STAMPS[1])
        # chunk `first` as dwell 0 of an attempt: the K = 1 sequence starting there
        seq = oracle_dwell_sequence([x], c.codes, pfa, c.D, c.dmax, c.dstep, False, c.spc, fs=c.fs)
        thr = c.threshold(pfa, 1)
        exact = []
        for p in range(len(c.prns)):
            exact.append(check_dwell_record(recs[p], seq[p][0], pfa, 0, STAMPS[1], thr, c.dmax, c.dstep, c.spcode))
        assert all(exact[:c.nvis]), exact
        one = acq.run(x, stamp0=STAMPS[1])[0]
        for p in range(len(c.prns)):
            _same_cell_or_tie(recs[p], one[p], seq[p][0], p < c.nvis)
            assert one[p]["num_dwells"] == 1 and one[p]["samplestamp"] == STAMPS[1]
        with pytest.raises(gsdr.GsdrError) as e:
            acq.run_dwell(x, 1)
        assert e.value.code == gsdr.GSDR_E_ARG
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
@pytest.mark.parametrize("name", ["bt8000", "bt12000"])
def test_bit_transition(name, pfa):
    """bit_transition forces max_dwells to 1: run_dwell(x, 0) keeps outputs [N/2, N) of the
    N-point transform; the peak-ratio window wraps at N while the row has N/2 entries.
    Satellite 0 peaks within samples_per_chip of the row's start, satellite 1 of its end
    (pinned on the oracle in test_oracle_acq_grid.py)."""
    c, acq = _handle(name, pfa, max_dwells=4)
    worst = {"peak": 0.0, "stat": 0.0, "aux": 0.0}
    for first in (0, 1):
        seq = c.seq(pfa, first)
        if pfa == 0:
            assert seq[0][0][0] < c.spc and seq[1][0][0] + c.spc >= c.N // 2
        recs = acq.run_dwell(c.chunks[first], 0, STAMPS[2 - first])
        _distances(recs, [s[0] for s in seq], pfa, worst)
        exact = c.check(recs, pfa, 0, STAMPS[2 - first], first)
        assert sum(exact) >= len(exact) - 1
        with pytest.raises(gsdr.GsdrError) as e:
            acq.run_dwell(c.chunks[first], 1)
        assert e.value.code == gsdr.GSDR_E_ARG
    _log("dwell_calls_bit_transition", name, pfa, worst)
    acq.close()


@pytest.mark.parametrize("item", [gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_integer_input(item):
    """cshort / ibyte blocks through run_dwell (N = 4000, two dwells): the engine converts
    the interleaved integer pairs exactly, so every call's records are byte-identical to
    the gr_complex run of the converted samples, which is checked against the oracle."""
    c, pfa, K = dwell_case("lds4000"), 0.01, 2
    xi = [synth.to_cshort(x, 2000.0) if item == gsdr.ITEM_CSHORT else synth.to_ibyte(x, 24.0) for x in c.chunks[:K]]
    xf = [(v[0::2].astype(np.float32) + 1j * v[1::2].astype(np.float32)).astype(np.complex64) for v in xi]
    acq = c.make(pfa, max_dwells=K, item_type=item)
    ref = c.make(pfa, max_dwells=K)
    seq = oracle_dwell_sequence(xf, c.codes, pfa, c.D, c.dmax, c.dstep, False, c.spc, fs=c.fs)
    for k in range(K):
        r = acq.run_dwell(xi[k], k, STAMPS[k])
        rf = ref.run_dwell(xf[k], k, STAMPS[k])
        assert r.tobytes() == rf.tobytes(), k
        exact = [check_dwell_record(r[p], seq[p][k], pfa, k, STAMPS[k], c.threshold(pfa, K), c.dmax, c.dstep,
                                    c.spcode) for p in range(len(c.prns))]
        assert all(exact[:c.nvis]), exact
    for h in (acq, ref):
        h.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_argument_checks(pfa):
    """dwell >= max_dwells is an argument error, a call before any code is set a state
    error; after either the handle runs a correct sequence."""
    c = dwell_case("lds4000")
    acq = gsdr.Acquisition(c.fs, c.N, c.dmax, c.dstep, pfa=pfa, max_prns=len(c.prns) + 2, max_dwells=c.K)
    acq.nprn = len(c.prns)  # room for the records the call must not write
    with pytest.raises(gsdr.GsdrError) as e:
        acq.run_dwell(c.chunks[0], 0)
    assert e.value.code == gsdr.GSDR_E_STATE
    acq.set_local_codes(c.codes, c.prns)
    if pfa == 0:
        acq.set_threshold(c.threshold(pfa))
    for bad in (c.K, c.K + 5):
        with pytest.raises(gsdr.GsdrError) as e:
            acq.run_dwell(c.chunks[0], bad)
        assert e.value.code == gsdr.GSDR_E_ARG
    r0 = acq.run_dwell(c.chunks[0], 0, STAMPS[0])
    c.check(r0, pfa, 0, STAMPS[0])
    with pytest.raises(gsdr.GsdrError) as e:  # a refused call inside an attempt
        acq.run_dwell(c.chunks[1], c.K)
    assert e.value.code == gsdr.GSDR_E_ARG
    for k in range(1, c.K):
        c.check(acq.run_dwell(c.chunks[k], k, STAMPS[k]), pfa, k, STAMPS[k])
    acq.close()

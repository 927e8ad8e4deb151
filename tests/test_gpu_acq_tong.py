"""Tong acquisition of the C ABI (gsdr_acq_set_tong, gsdr_acq_tong_reset, gsdr_acq_run_tong and its
ring form, gsdr_acq_dump_tong_grid: acq_pair_power_kernel and the scales, acq_tong_grid_kernel on
every kind of LDS plan with the running row in LDS and in HBM, acq_tong_update_kernel) against the
float64 restatement of pcps_tong_acquisition_cc in tests/tong_checks.py.

Inputs: tong_checks.CASES (N = 2000 and 4000 on compile-time plans, the latter a handle whose plain
search is packed; 3000 on a run-time plan; 16000, whose row does not fit beside the transform in
LDS), nine rows, two streams of eight items with three code slots each, tong_init_val 2,
tong_max_val 4, tong_max_dwells 8.  Three slots hold at most three paths, so the five the counter
has to show are spread over the two streams of a case: stream 1 a positive after two dwells, a
negative after two dwells of an absent PRN and an oscillation that tong_max_dwells cuts (its
satellite on the last row at delay N - 1); stream 2 a positive that falls on dwell 8 and is
overridden (the same code in two slots) and an up-down-up path that ends positive.

Conditions, asserted on the CPU before any comparison (tong_checks.assert_margins): every winner of
the restatement is MIN_MARGIN = 1e-3 above its runner-up and every statistic at least 5 % from
threshold * dwell.  Grids: every row within RTOL = 1e-4 of the grid's largest value; integers and
the delay exactly; mag and input power within 1e-4 of their value.  A sequence fed in
one call and in several gives byte-equal grids and records: the running row holds the same floats
whether it waits in LDS or in HBM."""
import ctypes
import json
import os

import numpy as np
import pytest

import gsdr
from gsdr import synth

import tong_checks as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = sorted(tc.CASES, key=lambda n: tc.CASES[n])
STAMP0 = 7_000_000_123
INTS = ("prn", "doppler_index", "indext", "doppler_hz", "samplestamp", "dwell_count", "tong_count", "state", "pad")
FLOATS = ("mag", "input_power")


def _handle(c, item_type=gsdr.ITEM_GR_COMPLEX, max_blocks=tc.NITEMS, max_prns=3, pfa=0.0, **kw):
    return gsdr.Acquisition(c.fs, c.n, c.dmax, c.dstep, pfa=pfa, max_prns=max_prns, max_blocks=max_blocks,
                            samples_per_code=float(c.spc), num_doppler_bins=c.D, fft_size=c.n, item_type=item_type,
                            **kw)


def _tong(c, stream=0, **kw):
    acq = _handle(c, **kw)
    acq.set_tong(tc.INIT, tc.TMAX, tc.MAX_DWELLS)
    acq.set_threshold(tc.THRESHOLD)
    _codes(acq, c, stream)
    return acq


def _codes(acq, c, stream):
    st = c.streams[stream]
    acq.set_local_codes(st["codes"], st["slots"])


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _check_records(c, out, refs, tag):
    """Device records [nitems, nslots] against the restatement's, a list per slot."""
    worst = 0.0
    for q, recs in enumerate(refs):
        tc.assert_margins(recs)
        for k, want in enumerate(recs):
            r = out[k, q]
            for f in INTS:
                assert int(r[f]) == want[f], (tag, k, q, f, r, want)
            assert float(r["acq_delay_samples"]) == want["acq_delay_samples"], (tag, k, q, r, want)
            for f in FLOATS:
                if want[f] == 0.0:
                    assert float(r[f]) == 0.0, (tag, k, q, f, r)
                else:
                    worst = max(worst, _rel(r[f], want[f]))
                    assert _rel(r[f], want[f]) <= tc.RTOL, (tag, k, q, f, float(r[f]), want[f])
    print("parity tong", json.dumps({"tag": tag, "case": c.name, "worst_rel": float("%.3g" % worst)}))


def _grid_err(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want)) / want.max())


@pytest.mark.parametrize("name", NAMES)
def test_records_of_both_streams(name):
    """(b), (c), (d): every field of every record of two eight-item calls, the PAST_END records behind
    each terminal item, the same code in two slots, and a reset of one slot."""
    c = tc.tong_case(name)
    acq = _tong(c)
    print("parity tong", json.dumps({"tag": "plan", "case": name, "plan": acq.plan, "reuse": acq.spectrum_reuse}))
    first = acq.run_tong(c.items(0)[0], nitems=tc.NITEMS, stamp0=STAMP0)
    assert first.shape == (tc.NITEMS, 3)
    _check_records(c, first, [c.reference(0, q, 0, tc.NITEMS, 0, STAMP0)[0] for q in range(3)], "stream 1")
    assert [int(s) for s in first[:, 0]["state"]] == [0, 1] + [3] * 6
    assert [int(s) for s in first[:, 1]["state"]] == [0, 2] + [3] * 6
    assert [int(s) for s in first[:, 2]["state"]] == [0] * 7 + [2]
    # every sequence has ended: a later call is past the end for all of them
    later = acq.run_tong(c.items(0)[0], nitems=2, stamp0=5)
    assert [int(s) for s in later["state"].reshape(-1)] == [3] * 6
    assert [(int(r["dwell_count"]), int(r["tong_count"])) for r in later[1]] == [(2, 4), (2, 0), (8, 2)]
    assert not later["mag"].any() and not later["indext"].any()
    # the reset of slot 0 restarts slot 0 alone, and its rows from zero
    acq.tong_reset([0])
    again = acq.run_tong(c.items(0)[0], nitems=2, stamp0=STAMP0)
    assert again[:, 0].tobytes() == first[:2, 0].tobytes()
    assert [int(s) for s in again[:, 1:]["state"].reshape(-1)] == [3] * 4
    # stream 2 on the same handle: new codes, every slot reset
    _codes(acq, c, 1)
    acq.tong_reset()
    second = acq.run_tong(c.items(1)[0], nitems=tc.NITEMS, stamp0=STAMP0)
    _check_records(c, second, [c.reference(1, q, 0, tc.NITEMS, 0, STAMP0)[0] for q in range(3)], "stream 2")
    assert [(int(r["tong_count"]), int(r["state"])) for r in second[:, 0]][-2:] == [(3, 0), (4, 2)]
    assert [int(s) for s in second[:, 1]["state"]] == [0, 0, 0, 1, 3, 3, 3, 3]
    # one code in two slots: equal records apart from the prn
    s0, s2 = second[:, 0].copy(), second[:, 2].copy()
    assert set(s0["prn"]) == {9} and set(s2["prn"]) == {31}
    s2["prn"] = s0["prn"]
    assert s0.tobytes() == s2.tobytes()
    acq.close()


@pytest.mark.parametrize("name", NAMES)
def test_grid_in_one_call_and_in_three(name):
    """(a): dump_tong_grid after one, two and three items, fed in one call and one call each."""
    c = tc.tong_case(name)
    acq = _tong(c)
    flat = c.items(0)[0]
    refs = [c.reference(0, q, 0, 3)[1] for q in range(3)]
    for q in range(3):
        assert not acq.dump_tong_grid(q).any()  # no item yet
    split = []
    for k in range(3):
        acq.run_tong(flat[k * c.n:(k + 1) * c.n], nitems=1, stamp0=k * c.n)
        split.append([acq.dump_tong_grid(q) for q in range(3)])
    for k in range(3):
        acq.tong_reset()
        acq.run_tong(flat, nitems=k + 1)
        # slots 0 and 1 end on item 2: their third item is speculation in one call and skipped in
        # three, so only the running slot 2 is compared after it
        for q in ((0, 1, 2) if k < 2 else (2,)):
            g = acq.dump_tong_grid(q)
            err = _grid_err(g, refs[q][k])
            print("parity tong", json.dumps({"tag": "grid", "case": name, "items": k + 1, "slot": q,
                                             "err_over_max": float("%.3g" % err)}))
            assert err <= tc.RTOL, (name, k, q, err)
            assert _grid_err(split[k][q], refs[q][k]) <= tc.RTOL
            assert g.tobytes() == split[k][q].tobytes(), (name, k, q)
    acq.close()


@pytest.mark.parametrize("name", ["t2000", "t16000"])
def test_split_calls_continue_the_sequences(name):
    """Eight items as calls of 3, 1 and 4 items: the records of one call of eight, byte for byte (the
    row in LDS and the row in HBM)."""
    c = tc.tong_case(name)
    acq = _tong(c, stream=1)
    flat = c.items(1)[0]
    whole = acq.run_tong(flat, nitems=tc.NITEMS, stamp0=STAMP0)
    acq.tong_reset()
    parts, k = [], 0
    for n in (3, 1, 4):
        parts.append(acq.run_tong(flat[k * c.n:(k + n) * c.n], nitems=n, stamp0=STAMP0 + k * c.n))
        k += n
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    acq.close()


@pytest.mark.parametrize("name,item_type", [("t2000", gsdr.ITEM_CSHORT), ("t3000", gsdr.ITEM_IBYTE),
                                            ("t4000", gsdr.ITEM_CSHORT), ("t16000", gsdr.ITEM_IBYTE)])
def test_integer_items(name, item_type):
    """(e): cshort and ibyte items, against the restatement on the converted samples."""
    c = tc.tong_case(name)
    acq = _tong(c, item_type=item_type)
    out = acq.run_tong(c.items(0, item_type)[0], nitems=tc.NITEMS, stamp0=3)
    _check_records(c, out, [c.reference(0, q, 0, tc.NITEMS, item_type, 3)[0] for q in range(3)],
                   "items%d" % item_type)
    acq.close()


@pytest.mark.parametrize("name", ["t3000", "t4000"])
def test_ring_form_equals_host_form(name):
    """(f): run_tong on a ring filled in uneven pushes from an absolute sample that is no multiple of the
    item: byte-equal to the host form."""
    c = tc.tong_case(name)
    acq = _tong(c)
    flat = c.items(0)[0]
    host = acq.run_tong(flat, nitems=tc.NITEMS, stamp0=STAMP0)
    first = 12345
    assert first % c.n != 0
    lead = synth.gps_l1_iq(c.fs, 777, [], seed_offset=9)
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=16 * c.n, max_window_items=tc.NITEMS * c.n)
    ring.push(lead, first - len(lead))
    pushed = 0
    for n in (1, 999, c.n + 3, len(flat)):
        n = min(n, len(flat) - pushed)
        ring.push(flat[pushed:pushed + n], first + pushed)
        pushed += n
    acq.tong_reset()
    got = acq.run_tong(ring, nitems=tc.NITEMS, stamp0=STAMP0, first_sample=first)
    assert got.tobytes() == host.tobytes()
    acq.tong_reset()
    with pytest.raises(gsdr.GsdrError):
        acq.run_tong(ring, nitems=tc.NITEMS, first_sample=first + 1)  # runs past the head
    again = acq.run_tong(ring, nitems=tc.NITEMS, stamp0=STAMP0, first_sample=first)
    assert again.tobytes() == host.tobytes()
    ring.close()
    acq.close()


@pytest.mark.parametrize("name,pfa", [("t4000", 0.01), ("t2000", 0.0), ("t16000", 0.01)])
def test_plain_run_is_unchanged(name, pfa):
    """(g): gsdr_acq_run on a handle after set_tong, and after Tong runs: the bytes of a fresh handle
    (CFAR on the packed plans, peak ratio on a compile-time plan)."""
    c = tc.tong_case(name)
    st = c.streams[0]
    x = c.items(0)[0][:3 * c.n]
    fresh = _handle(c, pfa=pfa)
    fresh.set_local_codes(st["codes"], st["slots"])
    want = fresh.run(x, nblocks=3, stamp0=11)
    fresh.close()
    acq = _handle(c, pfa=pfa)
    acq.set_tong(tc.INIT, tc.TMAX, tc.MAX_DWELLS)
    acq.set_local_codes(st["codes"], st["slots"])
    assert acq.run(x, nblocks=3, stamp0=11).tobytes() == want.tobytes()
    # the threshold is the handle's one, shared with the plain search: kept and put back
    thr = ctypes.c_float()
    assert gsdr.load().gsdr_acq_get_threshold(acq._h, ctypes.byref(thr)) == 0
    acq.set_threshold(tc.THRESHOLD)
    out = acq.run_tong(c.items(0)[0], nitems=tc.NITEMS, stamp0=STAMP0)
    _check_records(c, out, [c.reference(0, q, 0, tc.NITEMS, 0, STAMP0)[0] for q in range(3)], "pfa %g" % pfa)
    acq.set_threshold(thr.value)
    assert acq.run(x, nblocks=3, stamp0=11).tobytes() == want.tobytes()
    acq.close()


def test_errors_leave_the_handle_working():
    """(h): the argument, state and unsupported codes."""
    c = tc.tong_case("t2000")
    L = gsdr.load()
    flat = c.items(0)[0]
    out = np.zeros(tc.NITEMS * 3 + 4, gsdr.ACQ_TONG_RESULT_DTYPE)
    grid = np.zeros((c.D, c.n), np.float32)
    acq = _handle(c)
    h = acq._h
    # nothing configured yet
    assert L.gsdr_acq_run_tong(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    assert L.gsdr_acq_tong_reset(h, None, 0) == gsdr.GSDR_E_STATE
    assert L.gsdr_acq_dump_tong_grid(h, 0, gsdr._ptr(grid)) == gsdr.GSDR_E_STATE
    # init 0 (the reference's unsigned count wraps), init >= max (never meets '=='), no dwell allowed
    for init, tmax, maxd in ((0, 2, 3), (2, 2, 3), (5, 4, 8), (1, 2, 0)):
        assert L.gsdr_acq_set_tong(h, init, tmax, maxd) == gsdr.GSDR_E_ARG, (init, tmax, maxd)
    assert L.gsdr_acq_set_tong(None, 1, 2, 3) == gsdr.GSDR_E_ARG
    acq.set_tong(tc.INIT, tc.TMAX, tc.MAX_DWELLS)
    acq.set_threshold(tc.THRESHOLD)
    # configured, but no codes yet
    assert L.gsdr_acq_run_tong(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    _codes(acq, c, 0)
    good = acq.run_tong(flat, nitems=tc.NITEMS)
    _check_records(c, good, [c.reference(0, q)[0] for q in range(3)], "after errors")
    assert L.gsdr_acq_run_tong(h, None, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_tong(h, gsdr._ptr(flat), 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_tong(h, gsdr._ptr(flat), 0, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_tong(h, gsdr._ptr(flat), tc.NITEMS + 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_tong_stream(h, None, 0, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_tong_grid(h, 3, gsdr._ptr(grid)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_tong_grid(h, 0, None) == gsdr.GSDR_E_ARG
    bad = np.array([0, 3], np.uint32)
    assert L.gsdr_acq_tong_reset(h, gsdr._ptr(bad), 2) == gsdr.GSDR_E_ARG
    # none of these touched a sequence: still past the end; a carrier model other than exact is refused
    assert [int(s) for s in acq.run_tong(flat, nitems=1)["state"].reshape(-1)] == [3, 3, 3]
    acq.set_wipeoff("generic")
    assert L.gsdr_acq_run_tong(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_UNSUPPORTED
    assert b"exact" in L.gsdr_last_error()
    assert L.gsdr_acq_set_tong(h, 1, 2, 3) == gsdr.GSDR_E_UNSUPPORTED
    acq.set_wipeoff("exact")
    # the refused set_tong left the configuration: init 2, max 4, 8 dwells
    acq.tong_reset()
    assert acq.run_tong(flat, nitems=tc.NITEMS).tobytes() == good.tobytes()
    # an argument error of a configured handle leaves its configuration too
    assert L.gsdr_acq_set_tong(h, 0, 2, 3) == gsdr.GSDR_E_ARG
    acq.tong_reset()
    assert acq.run_tong(flat, nitems=tc.NITEMS).tobytes() == good.tobytes()
    acq.close()
    # a size with no one-launch LDS plan
    big = gsdr.Acquisition(25000000, 25000, 500, 250, max_prns=1, num_doppler_bins=5, fft_size=25000)
    assert big.plan["variant"] >= 20
    big.set_local_codes(synth.gps_ca_sampled(1, 25000000)[None, :], [1])
    x = synth.gps_l1_iq(25000000, 25000, [], seed_offset=3)
    before = big.run(x)
    assert L.gsdr_acq_set_tong(big._h, 1, 2, 3) == gsdr.GSDR_E_UNSUPPORTED
    assert b"one-launch" in L.gsdr_last_error()
    assert L.gsdr_acq_run_tong(big._h, gsdr._ptr(x), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    assert big.run(x).tobytes() == before.tobytes()
    big.close()
    # bit transition and dwell-accumulating handles serve no Tong, and keep serving plain runs
    st = c.streams[0]
    for kw in (dict(bit_transition=True), dict(max_dwells=2)):
        bt = gsdr.Acquisition(c.fs, c.n, c.dmax, c.dstep, pfa=0.01, max_prns=4, num_doppler_bins=c.D, **kw)
        bt.set_local_codes(st["codes"][:2], st["slots"][:2])
        x = flat[:bt.dwells * c.n]
        before = bt.run(x)
        assert L.gsdr_acq_set_tong(bt._h, 1, 2, 3) == gsdr.GSDR_E_UNSUPPORTED
        assert L.gsdr_acq_run_tong(bt._h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
        assert bt.run(x).tobytes() == before.tobytes()
        bt.close()


def test_capture():
    """(i): the committed GPS capture, PRN 1, +-10 kHz / 250 Hz, two 1 ms items with the adapters' default
    counter out of the way (tong_max_val 3): delay 524 at 1750 Hz after the first item and after both."""
    k = tc.capture_case()
    x = np.fromfile(os.path.join(GOLDEN, "GPS_L1_CA_ID_1_Fs_4Msps_2ms.dat"), np.complex64)
    thr = gsdr.tong_threshold(0.001, k["n"], 81)
    recs, grids = tc.sequence_records([x[:k["n"]], x[k["n"]:]], k["fs"], k["dmax"], k["dstep"], k["code"], k["spc"], thr,
                                      1, 3, 4)
    assert all(r["winner_margin"] >= tc.MIN_MARGIN and r["decision_margin"] >= tc.MIN_DECISION for r in recs)
    acq = gsdr.Acquisition(k["fs"], k["n"], k["dmax"], k["dstep"], max_prns=1, max_blocks=2, samples_per_code=4000.0,
                           num_doppler_bins=81, fft_size=k["n"])
    acq.set_tong(1, 3, 4)
    acq.set_threshold(thr)
    acq.set_local_codes(k["code"][None, :], [1])
    out = acq.run_tong(x, nitems=2)
    for b in range(2):
        r = out[b, 0]
        assert (int(r["doppler_index"]), int(r["doppler_hz"]), int(r["indext"]), float(r["acq_delay_samples"])) == \
            (47, 1750, 524, 524.0)
        assert (int(r["dwell_count"]), int(r["tong_count"]), int(r["state"])) == (b + 1, b + 2, b)
        for f in FLOATS:
            assert _rel(r[f], recs[b][f]) <= tc.RTOL, (b, f)
    err = _grid_err(acq.dump_tong_grid(0), grids[1])
    print("parity tong", json.dumps({"tag": "capture", "grid_err": float("%.3g" % err),
                                     "statistic": [float("%.4g" % float(s)) for s in out[:, 0]["mag"]],
                                     "threshold": thr}))
    assert err <= tc.RTOL
    acq.close()

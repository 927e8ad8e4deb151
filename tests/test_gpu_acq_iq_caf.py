"""E5a non-coherent IQ acquisition with CAF filter of the C ABI (gsdr_acq_set_iq_caf,
gsdr_acq_set_iq_codes, gsdr_acq_run_iq_caf and its ring form, gsdr_acq_dump_iq_caf_rows:
acq_iqcaf_replica_kernel, acq_iqcaf_grid_kernel on every kind of plan with the rows in LDS and in HBM,
acq_pair_power_kernel, acq_iqcaf_finish_kernel) against the float64 restatement of
galileo_e5a_noncoherent_iq_acquisition_caf_cc in tests/iq_caf_checks.py.

Inputs: iq_caf_checks.CASES -- N = 2000 (2 x 1000, compile-time plan), 3000 (3 x 1000, run-time
plan), 4000 with one component on a handle whose plain search is packed, 4000 zero padded, 8000 with
1 ms (the one slot pair fits LDS) and with 2 x 4000 (four rows do not), 16000 (2 x 8000, rows in HBM),
24000 (3 x 8000, generic four-step), 32000 (1 ms, packed four-step, nine rows), and 2000 with 21 rows
and the sign flipped at mid-item.  Two satellites, one present and one absent; two or three items whose
scenarios (both A forms, both B forms, I-B with Q-A, the case the quirk of :445 decides, satellites on
row 0 and row D - 1) are listed there.

Conditions, asserted on the CPU before any comparison (iq_caf_checks.assert_margins): on every row
both selection comparisons, Q-B's peak and the sum's peak, the grid's winner over the other rows and
the filter's maximum over the next row hold MIN_MARGIN = 1e-3; every statistic is 5 % from the
threshold.  Compared: choices exactly; the delay exactly and the raw index where it is pinned
(iq_caf_checks: periodic ties); peaks, mag, input power and statistic within RTOL = 1e-4."""
import json

import numpy as np
import pytest

import gsdr
from gsdr import synth

import iq_caf_checks as qc

pytestmark = pytest.mark.gpu

NAMES = sorted(qc.CASES, key=lambda n: (qc.CASES[n]["n"], n))
STAMP0 = 9_000_000_321


def _handle(c, item_type=gsdr.ITEM_GR_COMPLEX, max_prns=None, pfa=0.0, **kw):
    return gsdr.Acquisition(c.fs, c.n, c.dmax, c.dstep, pfa=pfa, max_prns=max_prns or 2 * c.nslots,
                            max_blocks=c.nitems, samples_per_code=float(c.spc), num_doppler_bins=c.D, fft_size=c.n,
                            item_type=item_type, **kw)


def _iq(c, window_hz, **kw):
    acq = _handle(c, **kw)
    acq.set_iq_caf(c.spc, c.ms, c.both, window_hz)
    acq.set_iq_codes(c.code_i, c.code_q, qc.PRNS)
    return acq


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _check_rows(c, got, rr, tag):
    """Device row records [D] of one (item, satellite) against the restatement's."""
    worst = 0.0
    for d, want in enumerate(rr):
        r = got[d]
        assert (int(r["choice_i"]), int(r["choice_q"])) == (want["choice_i"], want["choice_q"]), (tag, d, r, want)
        assert int(r["sum_index"]) % c.spc == want["sum_index"] % c.spc, (tag, d, r, want["sum_index"])
        if want["pinned"]:
            assert int(r["sum_index"]) == want["sum_index"], (tag, d, r, want["sum_index"])
        for f in ("peak_i", "peak_q", "sum_peak"):
            if want[f] == 0.0:
                assert float(r[f]) == 0.0, (tag, d, f, r)
            else:
                worst = max(worst, _rel(r[f], want[f]))
                assert _rel(r[f], want[f]) <= qc.RTOL, (tag, d, f, float(r[f]), want[f])
    return worst


def _check_record(c, r, want, tag):
    worst = 0.0
    for f in ("prn", "doppler_index", "caf_doppler_index", "doppler_hz", "caf_doppler_hz", "samplestamp"):
        assert int(r[f]) == want[f], (tag, f, r, want)
    assert float(r["acq_delay_samples"]) == want["acq_delay_samples"], (tag, r, want)
    assert int(r["indext"]) % c.spc == want["indext"] % c.spc, (tag, r, want)
    if want["pinned"]:
        assert int(r["indext"]) == want["indext"], (tag, r, want)
    assert float(r["pad"]) == 0.0
    for f in ("mag", "input_power", "test_statistic"):
        worst = max(worst, _rel(r[f], want[f]))
        assert _rel(r[f], want[f]) <= qc.RTOL, (tag, f, float(r[f]), want[f])
    return worst


def _check_all(c, acq, window_hz, item_type=0, tag=""):
    qc.assert_margins(c, window_hz, item_type)
    flat = c.items(item_type)[0]
    out = acq.run_iq_caf(flat, nitems=c.nitems, stamp0=STAMP0)
    assert out.shape == (c.nitems, len(qc.PRNS))
    ref = c.reference(window_hz, item_type, STAMP0)
    thr = c.threshold()
    worst = 0.0
    per = len(flat) // c.nitems
    for k in range(c.nitems):
        rows = acq.dump_iq_caf_rows(flat[k * per:(k + 1) * per])
        for s in range(len(qc.PRNS)):
            want, rr = ref[k][s]
            worst = max(worst, _check_rows(c, rows[s], rr, (c.name, tag, k, s)))
            worst = max(worst, _check_record(c, out[k, s], want, (c.name, tag, k, s)))
            # the present satellite is above the threshold, the absent one below, as in the restatement
            assert (float(out[k, s]["test_statistic"]) > thr) == (want["test_statistic"] > thr) == (s == 0)
    print("parity iq_caf", json.dumps({"case": c.name, "tag": tag, "window_hz": window_hz, "plan": acq.plan,
                                       "worst_rel": float("%.3g" % worst)}))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_records_against_the_restatement(name):
    """Row records and result records of every item and satellite, on every window of the case."""
    c = qc.iq_caf_case(name)
    qc.expectations(c)
    acq = _handle(c)
    outs = []
    for w in c.windows:
        acq.set_iq_caf(c.spc, c.ms, c.both, w)
        acq.set_iq_codes(c.code_i, c.code_q, qc.PRNS)
        outs.append(_check_all(c, acq, w))
    if name == "f2000":
        # the filter moves the Doppler, the two windows are told apart, and nothing else moves
        wide, narrow, off = outs
        for k in range(c.nitems):
            assert len({int(o[k, 0]["caf_doppler_index"]) for o in outs}) == 3
            assert int(off[k, 0]["caf_doppler_index"]) == int(off[k, 0]["doppler_index"])
        for o in (wide, narrow):
            o = o.copy()
            o["caf_doppler_index"], o["caf_doppler_hz"] = off["caf_doppler_index"], off["caf_doppler_hz"]
            assert o.tobytes() == off.tobytes()
    acq.close()


def test_the_plan_kinds_are_the_ones_meant():
    """The cases reach a compile-time, a run-time, a generic four-step and a packed four-step plan, and
    the handle of the one-component case runs its plain search packed."""
    want = {"q2000": range(1, 5), "q3000": range(10, 13), "q4000": range(1, 5), "q16000": range(1, 5),
            "q24000": range(20, 24), "p32000": range(24, 28)}
    for name, ids in want.items():
        c = qc.iq_caf_case(name)
        acq = _handle(c, pfa=0.01 if name == "q4000" else 0.0)
        assert acq.plan["variant"] in ids, (name, acq.plan)
        acq.close()


def test_quirk_is_kept():
    """On the quirk item Q-B's own peak is the larger on the satellite's row; the device, like :445,
    reads the I-B row at Q-B's index and keeps Q-A."""
    c = qc.iq_caf_case("q3000")
    k = [t["scenario"] for t in c.truth].index("quirk")
    row = c.truth[k]["row"]
    want = c.reference(c.windows[0])[k][0][1][row]
    assert want["true_choice_q"] == 1 and want["choice_q"] == 0
    assert want["forms"]["QB"][1] > 2.0 * want["forms"]["QA"][1]
    acq = _iq(c, c.windows[0])
    got = acq.dump_iq_caf_rows(c.x[k])[0][row]
    assert int(got["choice_q"]) == 0
    assert _rel(got["peak_q"], want["forms"]["QA"][1]) <= qc.RTOL
    acq.close()


@pytest.mark.parametrize("name", ["q2000", "q3000"])
def test_rows_in_hbm_equal_rows_in_lds(name, monkeypatch):
    """GSDR_ACQ_IQCAF_ROWS_HBM=1, read when a handle is created: the records and row records of the
    HBM form are the bytes of the LDS form's."""
    c = qc.iq_caf_case(name)
    got = {}
    for hbm in ("0", "1"):
        monkeypatch.setenv("GSDR_ACQ_IQCAF_ROWS_HBM", hbm)
        acq = _iq(c, c.windows[0])
        out = acq.run_iq_caf(c.items()[0], nitems=c.nitems, stamp0=5)
        rows = [acq.dump_iq_caf_rows(c.x[k]) for k in range(c.nitems)]
        got[hbm] = out.tobytes() + b"".join(r.tobytes() for r in rows)
        acq.close()
    assert got["0"] == got["1"]


@pytest.mark.parametrize("name", ["q3000", "q8000"])
def test_ring_form_equals_host_form(name):
    """run_iq_caf on a ring filled in uneven pushes from an absolute sample that is no multiple of the
    item: byte-equal to the host form."""
    c = qc.iq_caf_case(name)
    acq = _iq(c, c.windows[0])
    flat = c.items()[0]
    host = acq.run_iq_caf(flat, nitems=c.nitems, stamp0=STAMP0)
    first = 12345
    assert first % c.n != 0
    lead = synth.gps_l1_iq(c.fs, 777, [], seed_offset=9)
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=8 * c.n, max_window_items=c.nitems * c.n)
    ring.push(lead, first - len(lead))
    pushed = 0
    for n in (1, 999, c.n + 3, len(flat)):
        n = min(n, len(flat) - pushed)
        ring.push(flat[pushed:pushed + n], first + pushed)
        pushed += n
    got = acq.run_iq_caf(ring, nitems=c.nitems, stamp0=STAMP0, first_sample=first)
    assert got.tobytes() == host.tobytes()
    with pytest.raises(gsdr.GsdrError):
        acq.run_iq_caf(ring, nitems=c.nitems, first_sample=first + 1)  # runs past the head
    assert acq.run_iq_caf(ring, nitems=c.nitems, stamp0=STAMP0, first_sample=first).tobytes() == host.tobytes()
    ring.close()
    acq.close()


def test_cshort_items():
    """cshort items, against the restatement on the converted samples."""
    c = qc.iq_caf_case("q2000")
    acq = _iq(c, c.windows[0], item_type=gsdr.ITEM_CSHORT)
    _check_all(c, acq, c.windows[0], item_type=1, tag="cshort")
    acq.close()


def test_one_satellite_alone_and_in_company():
    """The present satellite searched alone gives the records it gives beside the absent one."""
    c = qc.iq_caf_case("q2000")
    acq = _iq(c, c.windows[0])
    both = acq.run_iq_caf(c.items()[0], nitems=c.nitems, stamp0=3)
    acq.set_iq_codes(c.code_i[:1], c.code_q[:1], qc.PRNS[:1])
    alone = acq.run_iq_caf(c.items()[0], nitems=c.nitems, stamp0=3)
    assert alone.shape == (c.nitems, 1)
    assert alone[:, 0].tobytes() == both[:, 0].tobytes()
    acq.close()


def test_errors_leave_the_handle_working():
    """The argument, state and unsupported codes."""
    c = qc.iq_caf_case("q2000")
    L = gsdr.load()
    flat = c.items()[0]
    out = np.zeros(c.nitems * 2 + 4, gsdr.ACQ_IQ_CAF_RESULT_DTYPE)
    rows = np.zeros((2, c.D), gsdr.ACQ_IQ_CAF_ROW_DTYPE)
    prns = np.array(qc.PRNS, np.uint32)
    ci, cq = np.ascontiguousarray(c.code_i), np.ascontiguousarray(c.code_q)
    acq = _handle(c)
    h = acq._h
    # nothing configured yet: codes before set, runs before both
    assert L.gsdr_acq_set_iq_codes(h, gsdr._ptr(ci), gsdr._ptr(cq), gsdr._ptr(prns), 2) == gsdr.GSDR_E_STATE
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    assert L.gsdr_acq_dump_iq_caf_rows(h, gsdr._ptr(flat), gsdr._ptr(rows)) == gsdr.GSDR_E_STATE
    # coherent_ms outside [1, 3], samples_per_code 0 and beyond the item
    for spc, ms in ((c.spc, 0), (c.spc, 4), (0, 2), (c.n + 1, 1)):
        assert L.gsdr_acq_set_iq_caf(h, spc, ms, 1, 0) == gsdr.GSDR_E_ARG, (spc, ms)
    # the window: below 2 steps CAF_bins_half is 0 (:605 divides by it); 2 half + 1 rows must fit the grid
    assert qc.window_error(2 * c.dstep - 1, c.dstep, c.D) and qc.window_error(2 * c.dstep * 5, c.dstep, c.D)
    assert not qc.window_error(2 * c.dstep * 4, c.dstep, c.D)
    assert L.gsdr_acq_set_iq_caf(h, c.spc, c.ms, 1, 2 * c.dstep - 1) == gsdr.GSDR_E_ARG
    assert b"CAF_bins_half" in L.gsdr_last_error()
    assert L.gsdr_acq_set_iq_caf(h, c.spc, c.ms, 1, 2 * c.dstep * 5) == gsdr.GSDR_E_ARG  # 11 rows > 9
    assert L.gsdr_acq_set_iq_caf(h, c.spc, c.ms, 1, 2 * c.dstep * 4) == gsdr.GSDR_OK     # 9 rows
    assert L.gsdr_acq_set_iq_caf(None, c.spc, c.ms, 1, 0) == gsdr.GSDR_E_ARG
    acq.set_iq_caf(c.spc, c.ms, c.both, c.windows[0])
    # configured, but no codes yet
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    # a four-slot satellite beyond max_prns (8 slots: two satellites), a missing Q row, null pointers
    three = np.array([1, 2, 3], np.uint32)
    ci3 = np.ascontiguousarray(np.concatenate([c.code_i, c.code_i[:1]]))
    assert L.gsdr_acq_set_iq_codes(h, gsdr._ptr(ci3), gsdr._ptr(ci3), gsdr._ptr(three), 3) == gsdr.GSDR_E_ARG
    assert b"slots" in L.gsdr_last_error()
    assert L.gsdr_acq_set_iq_codes(h, gsdr._ptr(ci), None, gsdr._ptr(prns), 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_iq_codes(h, None, gsdr._ptr(cq), gsdr._ptr(prns), 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_iq_codes(h, gsdr._ptr(ci), gsdr._ptr(cq), gsdr._ptr(prns), 0) == gsdr.GSDR_E_ARG
    acq.set_iq_codes(c.code_i, c.code_q, qc.PRNS)
    good = acq.run_iq_caf(flat, nitems=c.nitems, stamp0=STAMP0)
    for k in range(c.nitems):
        for s in range(2):
            _check_record(c, good[k, s], c.reference(c.windows[0], 0, STAMP0)[k][s][0], ("after errors", k, s))
    assert L.gsdr_acq_run_iq_caf(h, None, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), 0, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), c.nitems + 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_iq_caf_stream(h, None, 0, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_iq_caf_rows(h, gsdr._ptr(flat), None) == gsdr.GSDR_E_ARG
    # a plain run on the handle while it holds IQ-CAF slots
    plain = np.zeros(c.nitems * 8, gsdr.ACQ_RESULT_DTYPE)
    assert L.gsdr_acq_run(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(plain)) == gsdr.GSDR_E_STATE
    # a carrier model other than exact is refused
    acq.set_wipeoff("generic")
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_UNSUPPORTED
    assert b"exact" in L.gsdr_last_error()
    assert L.gsdr_acq_set_iq_caf(h, c.spc, c.ms, 1, 0) == gsdr.GSDR_E_UNSUPPORTED
    acq.set_wipeoff("exact")
    # none of the refusals touched the configuration
    assert acq.run_iq_caf(flat, nitems=c.nitems, stamp0=STAMP0).tobytes() == good.tobytes()
    # plain codes give the handle back to the plain search, and take it from this one
    acq.set_local_codes(c.code_i, qc.PRNS)
    assert acq.run(flat, nblocks=c.nitems).shape == (c.nitems, 2)
    assert L.gsdr_acq_run_iq_caf(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    acq.set_iq_codes(c.code_i, c.code_q, qc.PRNS)
    assert acq.run_iq_caf(flat, nitems=c.nitems, stamp0=STAMP0).tobytes() == good.tobytes()
    acq.close()
    # bit transition and dwell-accumulating handles serve no IQ-CAF, and keep serving plain runs
    for kw in (dict(bit_transition=True), dict(max_dwells=2)):
        bt = gsdr.Acquisition(c.fs, c.n, c.dmax, c.dstep, pfa=0.01, max_prns=8, num_doppler_bins=c.D, **kw)
        bt.set_local_codes(c.code_i, qc.PRNS)
        x = flat[:bt.dwells * c.n]
        before = bt.run(x)
        assert L.gsdr_acq_set_iq_caf(bt._h, c.spc, c.ms, 1, 0) == gsdr.GSDR_E_UNSUPPORTED
        assert L.gsdr_acq_run_iq_caf(bt._h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
        assert bt.run(x).tobytes() == before.tobytes()
        bt.close()


def test_plain_run_is_unchanged():
    """gsdr_acq_run on a handle before set_iq_caf and after the plain codes are restored: the same bytes
    (the packed plain search of N = 4000)."""
    c = qc.iq_caf_case("q4000")
    acq = _handle(c, pfa=0.01, max_prns=4)
    acq.set_local_codes(c.code_i, qc.PRNS)
    flat = c.items()[0]
    want = acq.run(flat, nblocks=c.nitems, stamp0=11)
    acq.set_iq_caf(c.spc, c.ms, c.both, c.windows[0])
    assert acq.run(flat, nblocks=c.nitems, stamp0=11).tobytes() == want.tobytes()  # set_iq_caf alone changes nothing
    acq.set_iq_codes(c.code_i, None, qc.PRNS)
    _check_all(c, acq, c.windows[0], tag="packed handle")
    acq.set_local_codes(c.code_i, qc.PRNS)
    assert acq.run(flat, nblocks=c.nitems, stamp0=11).tobytes() == want.tobytes()
    acq.close()

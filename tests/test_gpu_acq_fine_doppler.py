"""The fine-Doppler estimate of the C ABI (gsdr_acq_fine_doppler and its ring and dump forms:
acq_fine_kernel, acq_fine_finish_kernel) against the float64 restatement of
pcps_acquisition_fine_doppler_cc::estimate_Doppler in tests/fine_checks.py.

Inputs: fine_checks.CASES, built once per case -- one 10 ms window with three satellites whose
Dopplers are whole fine bins, and an absent PRN.  Every comparison first asserts, on the CPU,
that the restatement's best bin is MIN_MARGIN (1e-3) above its second best, then demands the
same index.  Spectra and peaks: within RTOL = 1e-4 of the spectrum's maximum."""
import json

import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import pcps

import fine_checks as fc

pytestmark = pytest.mark.gpu

NAMES = ["lds20000", "four20480", "four40000"]
# the 1024-lane four-step instance: 10 x 16000, and 25 x 10000 (whose peaks lie where the double
# and the all-float frequency formulas differ, fine_checks.CASES)
BIG = ["four160000", "four250000"]


def _handle(c, **kw):
    return gsdr.Acquisition(c.fs, c.N, 5000, 250, pfa=0.0, max_prns=4, **kw)


def _check_records(c, out, idx, item_type=0, coarse=None, tag=""):
    """out[j] against the restatement of request idx[j]."""
    worst = 0.0
    for j, i in enumerate(idx):
        ref = c.reference(i, item_type, None if coarse is None else coarse[j])
        assert ref["margin"] >= fc.MIN_MARGIN, (c.name, i, ref["margin"])
        r = out[j]
        rel = abs(float(r["peak"]) - ref["peak"]) / ref["peak"]
        worst = max(worst, rel)
        print("parity fine", json.dumps({"tag": tag, "case": c.name, "req": i, "index": int(r["index"]),
                                         "ref_index": ref["index"], "peak_rel": float("%.3g" % rel)}))
        assert int(r["index"]) == ref["index"], (c.name, i, int(r["index"]), ref["index"])
        assert np.float32(r["freq_hz"]).tobytes() == np.float32(ref["freq_hz"]).tobytes(), (r["freq_hz"], ref["freq_hz"])
        assert int(r["accepted"]) == ref["accepted"]
        assert float(r["doppler_hz"]) == ref["doppler_hz"]
        assert rel <= fc.RTOL, (c.name, i, rel)
        assert int(r["pad"]) == 0
    return worst


@pytest.mark.parametrize("name", NAMES + BIG[:1])
def test_every_bin(name):
    """dump_fine_spectrum, all 80 N bins, for each satellite's code phase (0, 1, 2, N - 1 and
    mid-row over the cases: the replica alignment with its quirk shows in every bin)."""
    c = fc.fine_case(name)
    acq = _handle(c)
    assert acq.fine_plan == c.plan, acq.fine_plan
    for i in range(3):
        shift, _, slot = c.requests[i]
        ref = c.reference(i)
        assert ref["margin"] >= fc.MIN_MARGIN
        spec = acq.dump_fine_spectrum(c.x, c.codes[slot], shift)
        assert spec.shape == (c.M,) and spec.dtype == np.float32
        err = float(np.max(np.abs(spec.astype(np.float64) - ref["spectrum"])) / ref["peak"])
        print("parity fine", json.dumps({"tag": "every_bin", "case": name, "req": i, "max_err_over_peak": float("%.3g" % err)}))
        assert err <= fc.RTOL, (name, i, err)
        assert int(np.argmax(spec)) == ref["index"]
    acq.close()


@pytest.mark.parametrize("name", NAMES + BIG)
def test_results(name):
    """index, freq_hz (bit-equal), accepted, doppler_hz and the peak for the three satellites
    in one call: a peak in every residue class of the bin index mod 8 over the cases, peaks
    at negative frequencies (index >= M / 2) among them."""
    c = fc.fine_case(name)
    acq = _handle(c)
    out = acq.fine_doppler(c.x, c.codes, c.requests[:3])
    _check_records(c, out, [0, 1, 2], tag="results")
    acq.close()


@pytest.mark.parametrize("name", NAMES)
def test_batch_with_absent_prn(name):
    """One call, three requests: two PRNs of the window and one that is absent (its record is
    the restatement's too: the first maximum of a noise spectrum, not accepted)."""
    c = fc.fine_case(name)
    acq = _handle(c)
    idx = [0, 1, 3]
    out = acq.fine_doppler(c.x, c.codes, [c.requests[i] for i in idx])
    _check_records(c, out, idx, tag="batch")
    assert int(out[2]["accepted"]) == 0 and float(out[2]["doppler_hz"]) == c.requests[3][1]
    # the same requests in another order, one code row only: records follow their requests
    sub = np.ascontiguousarray(c.codes[[1]])
    one = acq.fine_doppler(c.x, sub, [(c.requests[1][0], c.requests[1][1], 0)])
    assert one.tobytes() == out[1:2].tobytes()
    acq.close()


def test_rejected_estimate():
    """coarse_doppler_hz = true + 1250: not accepted, doppler_hz stays the coarse value."""
    c = fc.fine_case("four40000")
    acq = _handle(c)
    coarse = [c.reference(i)["doppler_hz"] + 1250.0 for i in range(3)]
    reqs = [(c.requests[i][0], coarse[i], c.requests[i][2]) for i in range(3)]
    out = acq.fine_doppler(c.x, c.codes, reqs)
    _check_records(c, out, [0, 1, 2], coarse=coarse, tag="rejected")
    for i in range(3):
        assert int(out[i]["accepted"]) == 0 and float(out[i]["doppler_hz"]) == coarse[i]
    acq.close()


@pytest.mark.parametrize("item_type", [gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_item_types(item_type):
    """The 4 Msps case as cshort and ibyte items, against the restatement on the converted
    samples: every bin of one spectrum, and the records of all four requests."""
    c = fc.fine_case("four40000")
    acq = _handle(c, item_type=item_type)
    raw, _ = c.items(item_type)
    shift, _, slot = c.requests[0]
    ref = c.reference(0, item_type)
    assert ref["margin"] >= fc.MIN_MARGIN
    spec = acq.dump_fine_spectrum(raw, c.codes[slot], shift)
    err = float(np.max(np.abs(spec.astype(np.float64) - ref["spectrum"])) / ref["peak"])
    assert err <= fc.RTOL, err
    out = acq.fine_doppler(raw, c.codes, c.requests)
    _check_records(c, out, [0, 1, 2, 3], item_type=item_type, tag="item%d" % item_type)
    acq.close()


@pytest.mark.parametrize("name", ["lds20000", "four40000"])
def test_ring_form_equals_host_form(name):
    """fine_doppler_stream on a ring filled in uneven pushes, the window starting at an
    absolute sample that is no multiple of the block: records byte-equal to the host form."""
    c = fc.fine_case(name)
    acq = _handle(c)
    host = acq.fine_doppler(c.x, c.codes, c.requests)
    first = 12345
    lead = synth.gps_l1_iq(c.fs, 777, [], seed_offset=9)  # noise ahead of the window
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=16 * c.N, max_window_items=10 * c.N)
    ring.push(lead, first - len(lead))
    pushed = 0
    for n in (1, 999, c.N + 3, 5 * c.N - 17, c.L):
        n = min(n, c.L - pushed)
        ring.push(c.x[pushed:pushed + n], first + pushed)
        pushed += n
    assert pushed == c.L
    got = acq.fine_doppler_stream(ring, first, c.codes, c.requests)
    assert got.tobytes() == host.tobytes()
    with pytest.raises(gsdr.GsdrError):
        acq.fine_doppler_stream(ring, first + 1, c.codes, c.requests)  # runs past the head
    again = acq.fine_doppler_stream(ring, first, c.codes, c.requests)
    assert again.tobytes() == host.tobytes()
    ring.close()
    acq.close()


def test_fine_call_between_two_dwells():
    """A fine-Doppler call between dwell 0 and dwell 1 of run_dwell leaves the later dwell's
    records as they are without it."""
    c = fc.fine_case("four40000")
    kw = dict(max_dwells=2, num_doppler_bins=40)
    blocks = [c.x[:c.N], c.x[c.N:2 * c.N]]
    plain = _handle(c, **kw)
    plain.set_local_codes(c.codes, c.prns)
    want = [plain.run_dwell(blocks[k], k, 100 + k).copy() for k in range(2)]
    plain.close()
    acq = _handle(c, **kw)
    acq.set_local_codes(c.codes, c.prns)
    d0 = acq.run_dwell(blocks[0], 0, 100).copy()
    out = acq.fine_doppler(c.x, c.codes, c.requests[:3])
    d1 = acq.run_dwell(blocks[1], 1, 101).copy()
    assert d0.tobytes() == want[0].tobytes() and d1.tobytes() == want[1].tobytes()
    _check_records(c, out, [0, 1, 2], tag="interleaved")
    acq.close()


def test_plan_built_at_create(monkeypatch):
    """GSDR_ACQ_FINE=1: gsdr_acq_create builds the plan and its buffers (fine_ready from the
    start); without it the first call does.  The records are the same, and a size without a fine
    plan still gives a handle, never ready."""
    c = fc.fine_case("four20480")
    monkeypatch.delenv("GSDR_ACQ_FINE", raising=False)
    lazy = _handle(c)
    assert lazy.fine_ready is False
    want = lazy.fine_doppler(c.x, c.codes, c.requests)
    assert lazy.fine_ready is True
    lazy.close()
    monkeypatch.setenv("GSDR_ACQ_FINE", "1")
    acq = _handle(c)
    assert acq.fine_ready is True
    assert acq.fine_doppler(c.x, c.codes, c.requests).tobytes() == want.tobytes()
    acq.close()
    bt = gsdr.Acquisition(c.fs, c.N, 5000, 250, pfa=0.0, max_prns=4, bit_transition=True)
    assert bt.fine_ready is False
    with pytest.raises(gsdr.GsdrError) as e:
        bt.fine_plan
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED
    bt.close()


def test_scratch_pool_grows_with_the_batch():
    """The four-step pool starts at 32 rows (four requests' workgroups); a call with more
    requests grows it to its bound of 64, and both before and after the records are the same."""
    c = fc.fine_case("four40000")
    acq = _handle(c)
    few = acq.fine_doppler(c.x, c.codes, c.requests)
    many = acq.fine_doppler(c.x, c.codes, c.requests * 3)
    again = acq.fine_doppler(c.x, c.codes, c.requests)
    for j in range(3):
        assert many[4 * j:4 * j + 4].tobytes() == few.tobytes()
    assert again.tobytes() == few.tobytes()
    _check_records(c, few, [0, 1, 2, 3], tag="pool")
    acq.close()


def test_errors_leave_the_handle_usable():
    c = fc.fine_case("lds20000")
    # fs = 2.1 Msps (L = 21000 has a factor 7): N = 2100 has the factor too, so the handle's own
    # FFT has no plan and gsdr_acq_create is what answers GSDR_E_UNSUPPORTED; no handle exists
    with pytest.raises(gsdr.GsdrError) as e:
        gsdr.Acquisition(2100000, 2100, 5000, 250, max_prns=1)
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED
    # the fine planner's own rejection needs a size the coarse stage plans (64000 = 16 x 4000)
    # whose 10 ms transform fits no engine (640000 > 25 x 20352); the handle stays usable
    big = gsdr.Acquisition(64000000, 64000, 250, 250, pfa=0.0, max_prns=1)
    assert big.plan["r1"] == 16
    with pytest.raises(gsdr.GsdrError) as e:
        big.fine_plan
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED
    with pytest.raises(gsdr.GsdrError) as e:
        big.fine_doppler(np.zeros(640000, np.complex64), np.ones((1, 64000), np.complex64), [(0, 0.0, 0)])
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED and big.fine_ready is False
    rng = np.random.default_rng(5)
    code = np.sign(rng.standard_normal(64000)).astype(np.complex64)
    noise = (rng.standard_normal(64000) + 1j * rng.standard_normal(64000)).astype(np.complex64)
    big.set_local_codes(code[None, :], [9])
    x = noise + np.roll(code, 321)
    rec = big.run(x)[0][0]
    M = pcps.magnitude_grid(x, pcps.doppler_wipeoffs(64000000, 64000, 250, 250, 2), pcps.fft_code(code, 64000, 64000))
    ti, di = pcps.max_to_input_power_statistic(M)[:2]
    assert (int(rec["prn"]), int(rec["code_phase"]), int(rec["doppler_index"])) == (9, int(ti), int(di))
    big.close()
    # bit transition, and consumed_samples != fft_size: 1 ms blocks only
    for kw in (dict(bit_transition=True), dict(fft_size=2 * c.N)):
        h = gsdr.Acquisition(c.fs, c.N, 5000, 250, pfa=0.0, max_prns=4, **kw)
        n = h.fft_size
        with pytest.raises(gsdr.GsdrError) as e:
            h.fine_doppler(np.zeros(10 * n, np.complex64), np.ones((1, n), np.complex64), [(0, 0.0, 0)])
        assert e.value.code == gsdr.GSDR_E_UNSUPPORTED, kw
        h.set_local_codes(np.stack([np.resize(row, h.conf.consumed_samples) for row in c.codes]), c.prns)
        assert len(h.run(c.x[:h.conf.consumed_samples])[0]) == 4
        h.close()
    # argument errors, then the same handle answers
    acq = _handle(c)
    for bad in ([(c.N, 0.0, 0)], [(0, 0.0, 4)], []):
        with pytest.raises(gsdr.GsdrError) as e:
            acq.fine_doppler(c.x, c.codes, bad)
        assert e.value.code == gsdr.GSDR_E_ARG, bad
    out = acq.fine_doppler(c.x, c.codes, c.requests[:1])
    _check_records(c, out, [0], tag="after_errors")
    acq.close()

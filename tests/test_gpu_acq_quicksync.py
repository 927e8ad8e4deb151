"""QuickSync acquisition of the C ABI (gsdr_acq_set_quicksync, gsdr_acq_set_quicksync_codes,
gsdr_acq_run_quicksync and its ring and dump forms: the code fold, acq_forward_fold_kernel /
acq_forward_fold_pk_kernel, acq_pair_power_kernel over an item, acq_quick_candidate_kernel and
acq_quick_merge_kernel around the engine's correlate and reduce kernels) against the float64
restatement of pcps_quicksync_acquisition_cc in tests/quicksync_checks.py.

Inputs: quicksync_checks.CASES, one per FFT plan and folding factor, built once.  Every comparison
of a row, folded phase or candidate first asserts, on the CPU, that the restatement's winner is
MIN_MARGIN (1e-3) above its runner-up.  Rows and candidate powers: within RTOL = 1e-4 of the
largest; mag, input power, statistic and candidate power: within 1e-4 of their value
(DESIGN.md 3)."""
import json
import os

import numpy as np
import pytest

import gsdr
from gsdr import synth

import quicksync_checks as qc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = sorted(qc.CASES, key=lambda n: (qc.CASES[n]["spc"] * qc.CASES[n]["p"], n))
STAMP0 = 7_000_000_123
FLOATS = ("mag", "input_power", "test_statistic", "candidate_power")


def _handle(c, item_type=gsdr.ITEM_GR_COMPLEX, max_blocks=qc.NITEMS, pfa=0.0, max_prns=None, nf=None, **kw):
    nf = c.nf if nf is None else nf
    return gsdr.Acquisition(c.fs, nf, c.dmax, c.dstep, pfa=pfa, max_prns=max_prns or len(c.prns),
                            max_blocks=max_blocks, samples_per_code=float(c.spc), num_doppler_bins=c.D, fft_size=nf,
                            item_type=item_type, **kw)


def _quick(c, **kw):
    acq = _handle(c, **kw)
    acq.set_quicksync(c.p, c.spc)
    acq.set_quicksync_codes(c.codes, c.prns)
    return acq


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _check_record(c, r, ref, tag):
    """One device record against the restatement's item_record."""
    want, m = ref["rec"], ref["margins"]
    assert min(m.values()) >= qc.MIN_MARGIN, (tag, m)
    rels = {k: _rel(r[k], want[k]) for k in FLOATS}
    print("parity quicksync", json.dumps({"tag": tag, "case": c.name, "row": int(r["doppler_index"]),
                                          "phase": int(r["folded_phase"]), "candidate": int(r["candidate"]),
                                          **{k: float("%.3g" % v) for k, v in rels.items()}}))
    for k in ("doppler_index", "folded_phase", "candidate", "doppler_hz", "samplestamp"):
        assert int(r[k]) == want[k], (tag, k, r, want)
    assert float(r["acq_delay_samples"]) == want["acq_delay_samples"], (tag, r, want)
    assert int(r["pad"]) == 0
    for k, v in rels.items():
        assert v <= qc.RTOL, (tag, k, v)


@pytest.mark.parametrize("name", NAMES)
def test_rows_candidates_and_records(name):
    """dump_quicksync: every Doppler row of every slot, the winner's p candidate powers.
    run_quicksync: every field of every (item, slot) record, three items in one call; the same
    items in three calls, byte for byte."""
    c = qc.quick_case(name)
    acq = _quick(c)
    assert acq.nprn == len(c.prns) and acq.fft_size == c.nf
    print("parity quicksync", json.dumps({"tag": "plan", "case": name, "plan": acq.plan,
                                          "reuse": acq.spectrum_reuse}))
    rows, cand = acq.dump_quicksync(c.x[0])
    assert rows.shape == (c.D, len(c.prns)) and cand.shape == (len(c.prns), c.p)
    for q in range(len(c.prns)):
        ref = c.reference(0, q)
        assert min(ref["margins"].values()) >= qc.MIN_MARGIN
        err = float(np.max(np.abs(rows[:, q].astype(np.float64) - ref["mags"])) / ref["mags"].max())
        cerr = float(np.max(np.abs(cand[q].astype(np.float64) - ref["cand"])) / ref["cand"].max())
        print("parity quicksync", json.dumps({"tag": "rows", "case": name, "slot": q,
                                              "rows_err_over_peak": float("%.3g" % err),
                                              "cand_err_over_max": float("%.3g" % cerr)}))
        assert err <= qc.RTOL, (name, q, err)
        assert cerr <= qc.RTOL, (name, q, cerr)
    flat = c.items()[0]
    out = acq.run_quicksync(flat, nitems=qc.NITEMS, stamp0=STAMP0)
    assert out.shape == (qc.NITEMS, len(c.prns))
    for b in range(qc.NITEMS):
        for q, prn in enumerate(c.prns):
            assert int(out[b, q]["prn"]) == prn
            _check_record(c, out[b, q], c.reference(b, q, 0, STAMP0), "records b%d q%d" % (b, q))
        one = acq.run_quicksync(c.x[b], nitems=1, stamp0=STAMP0 + b * c.L)
        assert one.tobytes() == out[b:b + 1].tobytes(), (name, b)
    acq.close()


def test_capture():
    """The committed GPS capture, PRN 1, +-10 kHz / 250 Hz: 81 rows on 8 stored spectra (the rows
    fs / Nf = 2000 Hz apart share one), so the winner, row 47, is a shifted window of stored row 7
    and its candidate check runs on the stored wipe-off times the shift's phasor."""
    k = qc.capture_case()
    x = np.fromfile(os.path.join(GOLDEN, "GPS_L1_CA_ID_1_Fs_4Msps_2ms.dat"), np.complex64)
    ref = qc.item_record(x, k["fs"], k["dmax"], k["dstep"], k["code"], k["p"], 0)
    assert min(ref["margins"].values()) >= qc.MIN_MARGIN, ref["margins"]
    acq = gsdr.Acquisition(k["fs"], 2000, k["dmax"], k["dstep"], max_prns=1, samples_per_code=4000.0,
                           num_doppler_bins=81, fft_size=2000)
    assert acq.spectrum_reuse == (8, 1)
    acq.set_quicksync(2, 4000)
    acq.set_quicksync_codes(k["code"][None, :], [1])
    r = acq.run_quicksync(x)[0, 0]
    assert (int(r["doppler_index"]), int(r["doppler_hz"]), float(r["acq_delay_samples"])) == (47, 1750, 524.0)
    assert (int(r["folded_phase"]), int(r["candidate"])) == (524, 0)
    for f in FLOATS:
        assert _rel(r[f], ref["rec"][f]) <= qc.RTOL, f
    rows, cand = acq.dump_quicksync(x)
    err = float(np.max(np.abs(rows[:, 0].astype(np.float64) - ref["mags"])) / ref["mags"].max())
    cerr = float(np.max(np.abs(cand[0].astype(np.float64) - ref["cand"])) / ref["cand"].max())
    print("parity quicksync", json.dumps({"tag": "capture", "rows_err": float("%.3g" % err),
                                          "cand_err": float("%.3g" % cerr),
                                          "statistic": float("%.4g" % float(r["test_statistic"]))}))
    assert err <= qc.RTOL and cerr <= qc.RTOL
    acq.close()


@pytest.mark.parametrize("item_type", [gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_integer_items(item_type):
    """cshort and ibyte items, against the restatement on the converted samples."""
    c = qc.quick_case("q4000x2")
    raw, _ = c.items(item_type)
    acq = _quick(c, item_type=item_type)
    out = acq.run_quicksync(raw, nitems=qc.NITEMS, stamp0=3)
    for b in range(qc.NITEMS):
        for q in range(len(c.prns)):
            _check_record(c, out[b, q], c.reference(b, q, item_type, 3), "items%d b%d q%d" % (item_type, b, q))
    acq.close()


@pytest.mark.parametrize("name", ["q4000x4", "q8000x2"])
def test_ring_form_equals_host_form(name):
    """run_quicksync_stream on a ring filled in uneven pushes from an absolute sample that is no
    multiple of the item: byte-equal to the host form."""
    c = qc.quick_case(name)
    acq = _quick(c)
    flat = c.items()[0]
    host = acq.run_quicksync(flat, nitems=qc.NITEMS, stamp0=STAMP0)
    first = 12345
    assert first % c.L != 0
    lead = synth.gps_l1_iq(c.fs, 777, [], seed_offset=9)
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=8 * c.L, max_window_items=qc.NITEMS * c.L)
    ring.push(lead, first - len(lead))
    pushed = 0
    for n in (1, 999, c.L + 3, len(flat)):
        n = min(n, len(flat) - pushed)
        ring.push(flat[pushed:pushed + n], first + pushed)
        pushed += n
    got = acq.run_quicksync_stream(ring, first, nitems=qc.NITEMS, stamp0=STAMP0)
    assert got.tobytes() == host.tobytes()
    with pytest.raises(gsdr.GsdrError):
        acq.run_quicksync_stream(ring, first + 1, nitems=qc.NITEMS)  # runs past the head
    again = acq.run_quicksync_stream(ring, first, nitems=qc.NITEMS, stamp0=STAMP0)
    assert again.tobytes() == host.tobytes()
    ring.close()
    acq.close()


def test_ties():
    """One item submitted twice as two items: equal records apart from the stamp.  One code in
    two slots: equal records apart from the prn."""
    c = qc.quick_case("q4000x2")
    acq = _handle(c)
    acq.set_quicksync(c.p, c.spc)
    acq.set_quicksync_codes(np.stack([c.codes[0], c.codes[1], c.codes[0]]), [1, 4, 31])
    twice = np.concatenate([c.x[1], c.x[1]])
    out = acq.run_quicksync(twice, nitems=2, stamp0=500)
    assert out.shape == (2, 3)
    a, b = out[0].copy(), out[1].copy()
    assert [int(s) for s in a["samplestamp"]] == [500] * 3 and [int(s) for s in b["samplestamp"]] == [500 + c.L] * 3
    b["samplestamp"] = a["samplestamp"]
    assert a.tobytes() == b.tobytes()
    s0, s2 = out[0, 0].copy(), out[0, 2].copy()
    assert (int(s0["prn"]), int(s2["prn"])) == (1, 31)
    s2["prn"] = s0["prn"]
    assert s0.tobytes() == s2.tobytes()
    _check_record(c, out[0, 0], c.reference(1, 0, 0, 500 - c.L), "ties")
    # quicksync_decide on the two equal dwells
    rec, pos, n = gsdr.quicksync_decide(out[:, 0], 1e9, False, 2)
    assert (pos, n, int(rec["samplestamp"])) == (False, 2, 500 + c.L)
    rec, pos, n = gsdr.quicksync_decide(out[:, 0], 0.0, True, 2)
    assert (pos, n, int(rec["samplestamp"])) == (True, 2, 500 + c.L)
    acq.close()


def test_errors_leave_the_handle_working():
    c = qc.quick_case("q4000x2")
    L = gsdr.load()
    flat = c.items()[0]
    codes = np.ascontiguousarray(c.codes)
    prns = np.array(c.prns, np.uint32)
    out = np.zeros(qc.NITEMS * len(prns) + 4, gsdr.ACQ_QUICKSYNC_RESULT_DTYPE)
    acq = _handle(c)
    h = acq._h
    # nothing configured yet
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    assert L.gsdr_acq_set_quicksync_codes(h, gsdr._ptr(codes), gsdr._ptr(prns), len(prns)) == gsdr.GSDR_E_STATE
    # p = 1, p = 17, spc % p != 0, Nf != fft_size
    assert L.gsdr_acq_set_quicksync(h, 1, c.nf) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_quicksync(h, 17, 17 * c.nf) == gsdr.GSDR_E_ARG
    assert b"[2,16]" in L.gsdr_last_error()
    assert L.gsdr_acq_set_quicksync(h, 3, 3 * c.nf + 1) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_quicksync(h, 2, 2 * c.nf + 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_quicksync(h, 4, c.spc) == gsdr.GSDR_E_ARG  # Nf 1000 on a handle of 2000
    assert L.gsdr_acq_set_quicksync(None, c.p, c.spc) == gsdr.GSDR_E_ARG
    # configured, but a run before the codes are set
    acq.set_quicksync(c.p, c.spc)
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    assert L.gsdr_acq_dump_quicksync(h, gsdr._ptr(flat), None, None) == gsdr.GSDR_E_STATE
    # null arguments, too many codes
    assert L.gsdr_acq_set_quicksync_codes(h, None, gsdr._ptr(prns), len(prns)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_quicksync_codes(h, gsdr._ptr(codes), None, len(prns)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_quicksync_codes(h, gsdr._ptr(codes), gsdr._ptr(prns), 0) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_quicksync_codes(h, gsdr._ptr(codes), gsdr._ptr(prns), len(prns) + 1) == gsdr.GSDR_E_ARG
    acq.set_quicksync_codes(codes, prns)
    good = acq.run_quicksync(flat, nitems=qc.NITEMS)
    for b in range(qc.NITEMS):
        for q in range(len(prns)):
            _check_record(c, good[b, q], c.reference(b, q), "after errors b%d q%d" % (b, q))
    assert L.gsdr_acq_run_quicksync(h, None, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), 0, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), qc.NITEMS + 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_quicksync_stream(h, None, 0, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_quicksync(h, None, None, None) == gsdr.GSDR_E_ARG
    # a wipe-off mode other than exact: unsupported for the run, and back
    acq.set_wipeoff("generic")
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_UNSUPPORTED
    assert b"exact" in L.gsdr_last_error()
    acq.set_wipeoff("exact")
    assert acq.run_quicksync(flat, nitems=qc.NITEMS).tobytes() == good.tobytes()
    # an error of a configured handle leaves its configuration
    assert L.gsdr_acq_set_quicksync(h, 17, 17 * c.nf) == gsdr.GSDR_E_ARG
    assert acq.run_quicksync(flat, nitems=qc.NITEMS).tobytes() == good.tobytes()
    # plain codes clear the mark
    acq.set_local_codes(codes[:, :c.nf], prns)
    assert L.gsdr_acq_run_quicksync(h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    acq.close()
    # a size with no one-launch LDS plan
    big = gsdr.Acquisition(25000000, 25000, 500, 250, max_prns=1, num_doppler_bins=5, fft_size=25000)
    assert big.plan["variant"] >= 20
    code = synth.gps_ca_sampled(1, 25000000)
    big.set_local_codes(code[None, :], [1])
    x = synth.gps_l1_iq(25000000, 25000, [], seed_offset=3)
    before = big.run(x)
    assert L.gsdr_acq_set_quicksync(big._h, 2, 50000) == gsdr.GSDR_E_UNSUPPORTED
    assert b"one-launch" in L.gsdr_last_error()
    assert L.gsdr_acq_run_quicksync(big._h, gsdr._ptr(x), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    assert big.run(x).tobytes() == before.tobytes()
    big.close()
    # bit transition and dwell-accumulating handles serve no QuickSync, and keep serving plain runs
    for kw in (dict(bit_transition=True), dict(max_dwells=2)):
        bt = gsdr.Acquisition(c.fs, c.nf, c.dmax, c.dstep, pfa=0.01, max_prns=4, num_doppler_bins=c.D, **kw)
        bt.set_local_codes(codes[:2, :c.nf], prns[:2])
        x = flat[:bt.dwells * c.nf]
        before = bt.run(x)
        assert L.gsdr_acq_set_quicksync(bt._h, c.p, c.spc) == gsdr.GSDR_E_UNSUPPORTED
        assert L.gsdr_acq_run_quicksync(bt._h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
        assert bt.run(x).tobytes() == before.tobytes()
        bt.close()


@pytest.mark.parametrize("name,pfa", [("q8000x2", 0.01), ("q4000x2", 0.0)])
def test_plain_run_is_unchanged(name, pfa):
    """gsdr_acq_run on a handle after set_quicksync, and after QuickSync runs: the bytes of a
    fresh handle (CFAR on the packed plan, peak ratio on a compile-time plan)."""
    c = qc.quick_case(name)
    plain = np.ascontiguousarray(c.codes[:, :c.nf])
    prns = np.array(c.prns, np.uint32)
    x = c.items()[0][:qc.NITEMS * c.nf]
    fresh = _handle(c, pfa=pfa)
    fresh.set_local_codes(plain, prns)
    want = fresh.run(x, nblocks=qc.NITEMS, stamp0=11)
    fresh.close()
    acq = _handle(c, pfa=pfa)
    acq.set_quicksync(c.p, c.spc)
    acq.set_local_codes(plain, prns)
    assert acq.run(x, nblocks=qc.NITEMS, stamp0=11).tobytes() == want.tobytes()
    acq.set_quicksync_codes(c.codes, prns)
    quick = acq.run_quicksync(c.items()[0], nitems=qc.NITEMS)
    for q in range(len(prns)):
        _check_record(c, quick[0, q], c.reference(0, q), "pfa %g q%d" % (pfa, q))
    acq.set_local_codes(plain, prns)
    assert acq.run(x, nblocks=qc.NITEMS, stamp0=11).tobytes() == want.tobytes()
    acq.close()


def test_modes_share_a_handle():
    """One handle moved QuickSync -> pairs -> plain (peak ratio) -> QuickSync: each mode's records
    are the bytes of a handle that ran only that mode, the two QuickSync runs are the same bytes,
    and a mode whose codes are not the ones in the slots is refused with GSDR_E_STATE.  The smallest
    shape on the packed forward (variant 62, N = 2000)."""
    c = qc.quick_case("q4000x2")
    assert len(c.prns) == 4
    prns = np.array(c.prns, np.uint32)
    plain = np.ascontiguousarray(c.codes[:, :c.nf])
    first, second, pair_prns = plain[0::2], plain[1::2], prns[0::2]
    flat = c.items()[0]
    x = flat[:qc.NITEMS * c.nf]

    def handle():
        return _handle(c, max_prns=4, max_blocks=qc.NITEMS)

    def refused(call):
        with pytest.raises(gsdr.GsdrError) as e:
            call()
        assert e.value.code == gsdr.GSDR_E_STATE, e.value
        return True

    only = handle()
    assert only.plan["variant"] < 20 and only.fft_size == 2000
    only.set_local_codes(plain, prns)
    want_plain = only.run(x, nblocks=qc.NITEMS, stamp0=STAMP0)
    only.close()
    only = handle()
    only.set_code_pairs(gsdr.PAIR_AS_IS, first, second, pair_prns)
    want_pairs = only.run_pairs(x, nblocks=qc.NITEMS, stamp0=STAMP0)
    only.close()
    only = _quick(c, max_prns=4)
    want_quick = only.run_quicksync(flat, nitems=qc.NITEMS, stamp0=STAMP0)
    only.close()
    assert want_plain.shape == (qc.NITEMS, 4) and want_pairs.shape == (qc.NITEMS, 2)
    assert want_quick.shape == (qc.NITEMS, 4)

    acq = handle()
    acq.set_quicksync(c.p, c.spc)
    acq.set_quicksync_codes(c.codes, prns)
    quick1 = acq.run_quicksync(flat, nitems=qc.NITEMS, stamp0=STAMP0)
    assert refused(lambda: acq.run_pairs(x, nblocks=qc.NITEMS))
    acq.set_code_pairs(gsdr.PAIR_AS_IS, first, second, pair_prns)
    pairs = acq.run_pairs(x, nblocks=qc.NITEMS, stamp0=STAMP0)
    assert refused(lambda: acq.run_quicksync(flat, nitems=qc.NITEMS))
    acq.set_local_codes(plain, prns)
    got_plain = acq.run(x, nblocks=qc.NITEMS, stamp0=STAMP0)
    assert refused(lambda: acq.run_pairs(x, nblocks=qc.NITEMS))
    assert refused(lambda: acq.run_quicksync(flat, nitems=qc.NITEMS))
    acq.set_quicksync_codes(c.codes, prns)
    quick2 = acq.run_quicksync(flat, nitems=qc.NITEMS, stamp0=STAMP0)
    acq.close()
    assert quick1.tobytes() == want_quick.tobytes()
    assert pairs.tobytes() == want_pairs.tobytes()
    assert got_plain.tobytes() == want_plain.tobytes()
    assert quick2.tobytes() == quick1.tobytes()


def test_doppler_grid_moved_after_configuring():
    """gsdr_acq_set_doppler rebuilds the wipe-off rows over the item too."""
    c = qc.quick_case("q4000x4")
    acq = gsdr.Acquisition(c.fs, c.nf, 2 * c.dmax, 2 * c.dstep, max_prns=len(c.prns), max_blocks=qc.NITEMS,
                           samples_per_code=float(c.spc), num_doppler_bins=c.D, fft_size=c.nf)
    acq.set_quicksync(c.p, c.spc)
    acq.set_quicksync_codes(c.codes, c.prns)
    acq.set_doppler(c.dmax, c.dstep)
    out = acq.run_quicksync(c.items()[0], nitems=qc.NITEMS)
    for q in range(len(c.prns)):
        _check_record(c, out[2, q], c.reference(2, q), "moved grid q%d" % q)
    acq.close()


def test_profiling_records_the_new_kernels_in_the_reduce_stage():
    c = qc.quick_case("q4000x2")
    acq = _quick(c)
    acq.set_profiling(True)
    acq.run(c.items()[0][:c.nf], nblocks=1)
    _, plain = acq.read_profile()
    acq.run_quicksync(c.items()[0], nitems=1)
    _, quick = acq.read_profile()
    assert quick[0] == plain[0] and quick[1] == plain[1], (plain, quick)
    assert quick[2] == plain[2] + 1 and quick[3] == 0, (plain, quick)
    acq.close()

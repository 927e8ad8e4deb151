"""Paired-code acquisition of the C ABI (gsdr_acq_set_code_pairs, gsdr_acq_run_pairs and its
ring and dump forms: acq_pair_replica_kernel, acq_pair_power_kernel, acq_pair_merge_kernel over
the engine's forward and correlate kernels) against the float64 restatement of
pcps_cccwsr_acquisition_cc and galileo_pcps_8ms_acquisition_cc in tests/pair_checks.py.

Inputs: pair_checks.CASES, one per FFT plan and kind, built once.  Every comparison of an index,
row or member first asserts, on the CPU, that the restatement's winner is MIN_MARGIN (1e-3) above
its runner-up.  Rows: within RTOL = 1e-4 of the grid maximum; mag, input power and statistic:
within 1e-4 of their value.  For the 8 ms members every row holds its maximum
twice, samples_per_code apart (pair_checks.member_rows): code_phase is compared mod
samples_per_code there, acq_delay_samples exactly."""
import ctypes
import json
import os

import numpy as np
import pytest

import gsdr
from gsdr import synth

import pair_checks as pc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = sorted(pc.CASES, key=lambda n: (pc.CASES[n]["N"], n))
STAMP0 = 7_000_000_123


def _handle(c, item_type=gsdr.ITEM_GR_COMPLEX, max_blocks=pc.NBLOCKS, pfa=0.0, npairs=None, **kw):
    npairs = len(c.prns) if npairs is None else npairs
    return gsdr.Acquisition(c.fs, c.N, c.dmax, c.dstep, pfa=pfa, max_prns=2 * npairs, max_blocks=max_blocks,
                            samples_per_code=float(c.spc), num_doppler_bins=c.D, fft_size=c.N, sampled_ms=4,
                            ms_per_code=4, item_type=item_type, **kw)


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def _check_record(c, r, ref, tag, member=True):
    """One device record against the restatement's block_record."""
    want, m = ref["rec"], ref["margins"]
    assert min(m["row"], m["index"]) >= pc.MIN_MARGIN and (not member or m["member"] >= pc.MIN_MARGIN), (tag, m)
    rels = {k: _rel(r[k], want[k]) for k in ("mag", "input_power", "test_statistic")}
    print("parity pairs", json.dumps({"tag": tag, "case": c.name, "row": int(r["doppler_index"]),
                                      "phase": int(r["code_phase"]), "member": int(r["member"]),
                                      **{k: float("%.3g" % v) for k, v in rels.items()}}))
    assert int(r["doppler_index"]) == want["doppler_index"], (tag, r, want)
    assert int(r["doppler_hz"]) == want["doppler_hz"]
    if c.policy == pc.PCPS_8MS:
        assert int(r["code_phase"]) % c.spc == want["code_phase"] % c.spc and int(r["code_phase"]) < c.N, (tag, r, want)
    else:
        assert int(r["code_phase"]) == want["code_phase"], (tag, r, want)
    if member:
        assert int(r["member"]) == want["member"], (tag, r, want)
    assert float(r["acq_delay_samples"]) == want["acq_delay_samples"]
    assert int(r["samplestamp"]) == want["samplestamp"]
    assert int(r["pad"]) == 0 and float(r["pad2"]) == 0.0
    for k, v in rels.items():
        assert v <= pc.RTOL, (tag, k, v)


@pytest.mark.parametrize("name", NAMES)
def test_rows_and_records(name):
    """dump_pair_rows: every Doppler row, both members.  run_pairs: every field of every (block,
    pair) record, three blocks in one call; the same blocks in three calls, record for record."""
    c = pc.pair_case(name)
    acq = _handle(c)
    acq.set_code_pairs(*c.args())
    assert acq.nprn == 2 * len(c.prns)
    rows = acq.dump_pair_rows(c.x[0])
    assert rows.shape == (c.D, len(c.prns), 2) and rows.dtype == np.float32
    for q in range(len(c.prns)):
        ref = c.reference(0, q)
        err = float(np.max(np.abs(rows[:, q, :].astype(np.float64) - ref["mags"])) / ref["mags"].max())
        print("parity pairs", json.dumps({"tag": "rows", "case": name, "pair": q, "max_err_over_peak": float("%.3g" % err)}))
        assert err <= pc.RTOL, (name, q, err)
    flat = c.items()[0]
    out = acq.run_pairs(flat, nblocks=pc.NBLOCKS, stamp0=STAMP0)
    assert out.shape == (pc.NBLOCKS, len(c.prns))
    for b in range(pc.NBLOCKS):
        for q, prn in enumerate(c.prns):
            assert int(out[b, q]["prn"]) == prn
            _check_record(c, out[b, q], c.reference(b, q, 0, STAMP0), "records b%d q%d" % (b, q))
        one = acq.run_pairs(c.x[b], nblocks=1, stamp0=STAMP0 + b * c.N)
        assert one.tobytes() == out[b:b + 1].tobytes(), (name, b)
    acq.close()


def test_equal_members_report_member_zero():
    """An exact tie inside every row: the two members are the same replica."""
    c = pc.pair_case("asis2000")
    acq = _handle(c)
    acq.set_code_pairs(gsdr.PAIR_AS_IS, c.first, c.first, np.array(c.prns, np.uint32))
    out = acq.run_pairs(c.items()[0], nblocks=pc.NBLOCKS)
    rows = acq.dump_pair_rows(c.x[0])
    assert np.array_equal(rows[:, :, 0], rows[:, :, 1])
    assert np.all(out["member"] == 0)
    for b in range(pc.NBLOCKS):
        for q in range(len(c.prns)):
            ref = c.reference(b, q)  # code A of the case is this pair's both members
            if ref["rec"]["member"] == 0:
                assert int(out[b, q]["doppler_index"]) == ref["rec"]["doppler_index"]
                assert _rel(out[b, q]["mag"], ref["rec"]["mag"]) <= pc.RTOL
    acq.close()


def test_same_block_twice_keeps_dwell_zero():
    """pair_decide with carry on one block given as two dwells: an exact tie between dwells."""
    c = pc.pair_case("sdj2000")
    acq = _handle(c)
    acq.set_code_pairs(*c.args())
    twice = np.concatenate([c.x[0], c.x[0]])
    out = acq.run_pairs(twice, nblocks=2, stamp0=500)
    for q in range(len(c.prns)):
        assert out[0, q]["mag"] == out[1, q]["mag"]
        rec, pos, n = gsdr.pair_decide(out[:, q], 1e9, carry_mag=True)
        assert (pos, n, int(rec["samplestamp"])) == (False, 2, 500)
        rec, pos, n = gsdr.pair_decide(out[:, q], 1e9, carry_mag=False)
        assert (pos, n, int(rec["samplestamp"])) == (False, 2, 500 + c.N)
    acq.close()


@pytest.mark.parametrize("item_type", [gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_integer_items(item_type):
    """cshort and ibyte items, against the restatement on the converted samples."""
    c = pc.pair_case("sdj2000")
    raw, _ = c.items(item_type)
    acq = _handle(c, item_type=item_type)
    acq.set_code_pairs(*c.args())
    out = acq.run_pairs(raw, nblocks=pc.NBLOCKS, stamp0=3)
    for b in range(pc.NBLOCKS):
        for q in range(len(c.prns)):
            _check_record(c, out[b, q], c.reference(b, q, item_type, 3), "items%d b%d q%d" % (item_type, b, q))
    acq.close()


@pytest.mark.parametrize("name", ["sdj4000", "asis32000"])
def test_ring_form_equals_host_form(name):
    """run_pairs_stream on a ring filled in uneven pushes from an absolute sample that is no
    multiple of the block: byte-equal to the host form."""
    c = pc.pair_case(name)
    acq = _handle(c)
    acq.set_code_pairs(*c.args())
    flat = c.items()[0]
    host = acq.run_pairs(flat, nblocks=pc.NBLOCKS, stamp0=STAMP0)
    first = 12345
    lead = synth.gps_l1_iq(c.fs, 777, [], seed_offset=9)
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=8 * c.N, max_window_items=pc.NBLOCKS * c.N)
    ring.push(lead, first - len(lead))
    pushed = 0
    for n in (1, 999, c.N + 3, len(flat)):
        n = min(n, len(flat) - pushed)
        ring.push(flat[pushed:pushed + n], first + pushed)
        pushed += n
    got = acq.run_pairs_stream(ring, first, nblocks=pc.NBLOCKS, stamp0=STAMP0)
    assert got.tobytes() == host.tobytes()
    with pytest.raises(gsdr.GsdrError):
        acq.run_pairs_stream(ring, first + 1, nblocks=pc.NBLOCKS)  # runs past the head
    again = acq.run_pairs_stream(ring, first, nblocks=pc.NBLOCKS, stamp0=STAMP0)
    assert again.tobytes() == host.tobytes()
    ring.close()
    acq.close()


def test_synthetic_e1_with_near_equal_members():
    """synth.gal_e1_iq: E1-B and E1-C share a carrier phase, so |plus| and |minus| are nearly
    equal.  mag and the statistic as everywhere; (row, phase) must be one of the two members'
    restatement cells; member only where its margin allows."""
    fs, N, dmax, dstep = 4000000, 16000, 1000, 250
    sats = [synth.GalileoSatellite(11, 250.0, 1000.25, 52.0, 0.7), synth.GalileoSatellite(19, -750.0, 3011.5, 50.0, 2.1)]
    x = synth.gal_e1_iq(fs, N, sats, seed_offset=5)
    prns = [11, 19, 30]
    codes = [pc.codes_for(p, N, N) for p in prns]
    first, second = np.stack([c[0] for c in codes]), np.stack([c[1] for c in codes])
    acq = gsdr.Acquisition(fs, N, dmax, dstep, max_prns=6, samples_per_code=float(N), num_doppler_bins=9, fft_size=N,
                           sampled_ms=4, ms_per_code=4)
    acq.set_code_pairs(gsdr.PAIR_SUM_DIFF_J, first, second, prns)
    out = acq.run_pairs(x, stamp0=9)[0]
    compared = 0
    for q in range(3):
        ref = pc.block_record(x, fs, dmax, dstep, pc.CCCWSR, first[q], second[q], N, 9)
        want, m = ref["rec"], ref["margins"]
        assert m["row"] >= pc.MIN_MARGIN and m["index"] >= pc.MIN_MARGIN, m
        r = out[q]
        d = int(r["doppler_index"])
        assert d == want["doppler_index"] and int(r["doppler_hz"]) == want["doppler_hz"]
        assert int(r["code_phase"]) in (int(ref["idx"][d, 0]), int(ref["idx"][d, 1])), (r, ref["idx"][d])
        assert int(r["code_phase"]) == int(ref["idx"][d, int(r["member"])])
        for k in ("mag", "input_power", "test_statistic"):
            assert _rel(r[k], want[k]) <= pc.RTOL, (q, k)
        assert int(r["samplestamp"]) == 9
        if m["member"] >= pc.MIN_MARGIN:
            compared += 1
            assert int(r["member"]) == want["member"]
            assert float(r["acq_delay_samples"]) == want["acq_delay_samples"]
        print("parity pairs", json.dumps({"tag": "synthetic", "pair": q, "member_margin": float("%.3g" % m["member"])}))
    # the two satellites in view sit where they were put
    assert [int(out[q]["doppler_hz"]) for q in range(2)] == [250, -750]
    acq.close()


@pytest.mark.parametrize("policy,sl,delay,doppler,member", [
    (pc.CCCWSR, slice(0, 16000), 2920, -750, 0), (pc.CCCWSR, slice(16000, 32000), 2920, -750, 0),
    (pc.PCPS_8MS, slice(0, 32000), 2920, -500, 1)])
def test_capture(policy, sl, delay, doppler, member):
    """The committed Galileo capture, PRN 1, +-10 kHz / 250 Hz (81 rows), on the device."""
    cap = np.fromfile(os.path.join(GOLDEN, "Galileo_E1_ID_1_Fs_4Msps_8ms.dat"), np.complex64)
    k = pc.capture_case(cap, policy)
    x = cap[sl]
    ref = pc.block_record(x, k["fs"], k["dmax"], k["dstep"], policy, k["first"], k["second"], k["spc"], 0)
    assert min(ref["margins"].values()) >= pc.MIN_MARGIN, ref["margins"]
    acq = gsdr.Acquisition(k["fs"], k["N"], k["dmax"], k["dstep"], max_prns=2, samples_per_code=float(k["spc"]),
                           num_doppler_bins=81, fft_size=k["N"], sampled_ms=4, ms_per_code=4)
    acq.set_code_pairs(gsdr.PAIR_SUM_DIFF_J if policy == pc.CCCWSR else gsdr.PAIR_AS_IS, k["first"][None, :],
                       k["second"][None, :], [1])
    r = acq.run_pairs(x)[0, 0]
    assert (float(r["acq_delay_samples"]), int(r["doppler_hz"]), int(r["member"])) == (delay, doppler, member)
    assert int(r["doppler_index"]) == ref["rec"]["doppler_index"]
    for f in ("mag", "input_power", "test_statistic"):
        assert _rel(r[f], ref["rec"][f]) <= pc.RTOL, f
    rows = acq.dump_pair_rows(x)
    err = float(np.max(np.abs(rows[:, 0, :].astype(np.float64) - ref["mags"])) / ref["mags"].max())
    print("parity pairs", json.dumps({"tag": "capture", "policy": policy, "rows_err": float("%.3g" % err),
                                      "statistic": float("%.4g" % float(r["test_statistic"]))}))
    assert err <= pc.RTOL
    acq.close()


@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_plain_run_is_unchanged(pfa):
    """run() before set_code_pairs, and after the codes are restored: byte-equal records (CFAR
    and peak-ratio handles)."""
    c = pc.pair_case("sdj4000")
    acq = _handle(c, pfa=pfa)
    plain = np.ascontiguousarray(c.first[:5])
    prns = np.array(c.prns[:5], np.uint32)
    acq.set_local_codes(plain, prns)
    flat = c.items()[0]
    before = acq.run(flat, nblocks=pc.NBLOCKS, stamp0=11)
    acq.set_code_pairs(*c.args())
    pairs = acq.run_pairs(flat, nblocks=pc.NBLOCKS)
    acq.set_local_codes(plain, prns)
    with pytest.raises(gsdr.GsdrError) as e:
        acq.run_pairs(flat, nblocks=pc.NBLOCKS)  # the mark is cleared
    assert e.value.code == gsdr.GSDR_E_STATE
    after = acq.run(flat, nblocks=pc.NBLOCKS, stamp0=11)
    assert after.tobytes() == before.tobytes()
    # and the pairs again give what they gave
    acq.set_code_pairs(*c.args())
    assert acq.run_pairs(flat, nblocks=pc.NBLOCKS).tobytes() == pairs.tobytes()
    acq.close()


def test_errors_leave_the_handle_working():
    c = pc.pair_case("sdj2000")
    L = gsdr.load()
    kind, first, second, prns = c.args()
    acq = _handle(c, npairs=2)  # max_prns = 4
    flat = c.items()[0]
    out = np.zeros(pc.NBLOCKS * 3, gsdr.ACQ_PAIR_RESULT_DTYPE)
    # no pairs yet
    assert L.gsdr_acq_run_pairs(acq._h, gsdr._ptr(flat), 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_STATE
    rows = np.zeros((c.D, 3, 2), np.float32)
    assert L.gsdr_acq_dump_pair_rows(acq._h, gsdr._ptr(flat), gsdr._ptr(rows)) == gsdr.GSDR_E_STATE
    # 2 npairs > max_prns, null pointers, an unknown kind
    assert L.gsdr_acq_set_code_pairs(acq._h, kind, gsdr._ptr(first), gsdr._ptr(second), gsdr._ptr(prns), 3) == gsdr.GSDR_E_ARG
    assert b"slots" in L.gsdr_last_error()
    assert L.gsdr_acq_set_code_pairs(acq._h, kind, None, gsdr._ptr(second), gsdr._ptr(prns), 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_code_pairs(acq._h, kind, gsdr._ptr(first), None, gsdr._ptr(prns), 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_code_pairs(acq._h, kind, gsdr._ptr(first), gsdr._ptr(second), None, 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_code_pairs(None, kind, gsdr._ptr(first), gsdr._ptr(second), gsdr._ptr(prns), 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_code_pairs(acq._h, 2, gsdr._ptr(first), gsdr._ptr(second), gsdr._ptr(prns), 2) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_code_pairs(acq._h, kind, gsdr._ptr(first), gsdr._ptr(second), gsdr._ptr(prns), 0) == gsdr.GSDR_E_ARG
    # the handle still works: two of the case's pairs
    acq.set_code_pairs(kind, first[:2], second[:2], prns[:2])
    good = acq.run_pairs(flat, nblocks=pc.NBLOCKS)
    for b in range(pc.NBLOCKS):
        for q in range(2):
            _check_record(c, good[b, q], c.reference(b, q), "after errors b%d q%d" % (b, q))
    assert L.gsdr_acq_run_pairs(acq._h, None, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_pairs(acq._h, gsdr._ptr(flat), 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_pairs(acq._h, gsdr._ptr(flat), pc.NBLOCKS + 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_pairs_stream(acq._h, None, 0, 1, 0, gsdr._ptr(out)) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_pair_rows(acq._h, gsdr._ptr(flat), None) == gsdr.GSDR_E_ARG
    assert acq.run_pairs(flat, nblocks=pc.NBLOCKS).tobytes() == good.tobytes()
    acq.close()
    # bit transition and dwell-accumulating handles serve no pairs, and keep serving plain runs
    for kw in (dict(bit_transition=True), dict(max_dwells=2)):
        bt = gsdr.Acquisition(c.fs, c.N, c.dmax, c.dstep, pfa=0.01, max_prns=4, num_doppler_bins=c.D, **kw)
        bt.set_local_codes(first[:2, :bt.conf.consumed_samples], prns[:2])
        x = np.tile(flat, 2)[:bt.dwells * bt.conf.consumed_samples]
        before = bt.run(x)
        assert L.gsdr_acq_set_code_pairs(bt._h, kind, gsdr._ptr(first), gsdr._ptr(second), gsdr._ptr(prns), 2) \
            == gsdr.GSDR_E_UNSUPPORTED
        assert L.gsdr_acq_run_pairs(bt._h, gsdr._ptr(x), 1, 0, gsdr._ptr(out)) in (gsdr.GSDR_E_UNSUPPORTED, gsdr.GSDR_E_STATE)
        assert bt.run(x).tobytes() == before.tobytes()
        bt.close()


def test_profiling_records_the_pair_kernels_in_the_reduce_stage():
    c = pc.pair_case("sdj2000")
    acq = _handle(c)
    acq.set_code_pairs(*c.args())
    acq.set_profiling(True)
    acq.run(c.items()[0], nblocks=1)
    _, plain = acq.read_profile()
    acq.run_pairs(c.items()[0], nblocks=1)
    _, pairs = acq.read_profile()
    assert pairs[2] == plain[2] + 1 and pairs[3] == 0, (plain, pairs)
    acq.close()

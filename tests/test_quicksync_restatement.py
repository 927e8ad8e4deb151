"""The float64 restatement of pcps_quicksync_acquisition_cc (tests/quicksync_checks.py) and the
host-side helpers of the QuickSync interface, without a GPU: the shared cases come out where their
satellites were planted with every margin above MIN_MARGIN, the committed capture gives the
reference's expected delay, the forward-spectrum reuse identity holds for the folded product, and
gsdr.quicksync_threshold / gsdr.quicksync_decide / the record's layout agree with the restatement
and the C compiler."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gsdr

import quicksync_checks as qc
from conftest import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(qc.CASES))
def test_cases_recover_the_planted_satellites(name):
    c = qc.quick_case(name)
    assert (c.nf, c.L) == (c.spc // c.p, c.p * c.spc)
    for b in range(qc.NITEMS):
        for q, (prn, present, row, tau) in enumerate(c.sats):
            ref = c.reference(b, q)
            assert min(ref["margins"].values()) >= qc.MIN_MARGIN, (name, b, prn, ref["margins"])
            if present:
                r = ref["rec"]
                assert (r["doppler_index"], r["acq_delay_samples"]) == (row, float(tau)), (name, b, prn, r)
                assert r["folded_phase"] == tau % c.nf and r["candidate"] == tau // c.nf


def test_last_satellite_reaches_the_last_row_candidate_and_phase():
    for name in qc.CASES:
        c = qc.quick_case(name)
        r = c.reference(0, 1)["rec"]
        assert (r["doppler_index"], r["folded_phase"], r["candidate"]) == (c.D - 1, c.nf - 1, c.p - 1)
        # the candidate's last read: sample 2 spc - 2 of the item
        assert int(r["acq_delay_samples"]) + c.spc - 1 == 2 * c.spc - 2 < c.L


def test_capture():
    """The reference's own test vector for this block: Doppler 1680 Hz, delay 524 samples."""
    k = qc.capture_case()
    x = np.fromfile(os.path.join(GOLDEN, "GPS_L1_CA_ID_1_Fs_4Msps_2ms.dat"), np.complex64)
    assert len(x) == k["p"] * k["spc"]
    ref = qc.item_record(x, k["fs"], k["dmax"], k["dstep"], k["code"], k["p"], 0)
    r, m = ref["rec"], ref["margins"]
    assert len(ref["mags"]) == 81
    assert (r["doppler_index"], r["doppler_hz"], r["folded_phase"], r["candidate"], r["acq_delay_samples"]) == \
        (47, 1750, 524, 0, 524.0)
    assert abs(r["test_statistic"] - 16.08) < 0.01
    assert m["row"] > 0.28 and m["index"] > 0.41 and m["candidate"] > 0.99, m


@pytest.mark.parametrize("name", ["q4000x2", "q12000x3"])
def test_reuse_identity(name):
    """fold(x w_{f + fs / Nf}) = fold(x w_f) exp(-2 pi i i / Nf): the segment offset k Nf drops out
    of the phase, so the rows fs / Nf apart share a forward spectrum, shifted by one bin."""
    c = qc.quick_case(name)
    x = c.x[0].astype(np.complex128)
    i = np.arange(c.nf, dtype=np.float64)
    for f in (-1000.0, 250.0):
        lo = qc.fold(x * qc.wipeoff(f, c.fs, c.L), c.nf)
        hi = qc.fold(x * qc.wipeoff(f + c.fs / c.nf, c.fs, c.L), c.nf)
        want = lo * np.exp(-2j * np.pi * i / c.nf)
        assert np.linalg.norm(hi - want) <= 1e-12 * np.linalg.norm(want)
        # and so the spectrum is the other's, one bin on
        assert np.linalg.norm(np.fft.fft(hi) - np.roll(np.fft.fft(lo), -1)) <= 1e-11 * np.linalg.norm(np.fft.fft(lo))


@pytest.mark.parametrize("pfa,spc,p,dmax,dstep", [(0.01, 4000, 4, 1000, 250), (0.001, 25000, 4, 5000, 250),
                                                  (0.1, 4000, 3, 10000, 500), (1e-6, 8000, 2, 0, 250)])
def test_threshold(pfa, spc, p, dmax, dstep):
    rows = len(range(-dmax, dmax + 1, dstep))
    ncells = (spc // p) * rows
    val = pow(1.0 - float(np.float32(pfa)), 1.0 / float(ncells))
    want = np.float32(-np.log(1.0 - val) / (float(spc) / float(p)))
    got = gsdr.quicksync_threshold(pfa, spc, p, dmax, dstep)
    assert abs(got - float(want)) <= 1e-6 * float(want)
    assert got == qc.threshold(pfa, spc, p, dmax, dstep)
    assert got == float(np.float32(got))
    with pytest.raises(AssertionError):
        gsdr.quicksync_threshold(pfa, spc, p, dmax, 0)


def _records(stats):
    rec = np.zeros(len(stats), gsdr.ACQ_QUICKSYNC_RESULT_DTYPE)
    rec["test_statistic"] = stats
    rec["samplestamp"] = np.arange(len(stats)) * 1000
    return rec


@pytest.mark.parametrize("bit_transition", [False, True])
@pytest.mark.parametrize("max_dwells", [1, 2, 3])
@pytest.mark.parametrize("stats", [(0.5, 3.0, 0.7), (3.0, 0.5, 0.7), (0.1, 0.2, 0.3), (0.1, 0.2, 3.0), (2.0,)])
def test_decide_equals_the_state_machine(stats, max_dwells, bit_transition):
    thr = 1.0
    rec, pos, n = gsdr.quicksync_decide(_records(stats), thr, bit_transition, max_dwells)
    want, wpos, wn = qc.decide([dict(test_statistic=float(np.float32(s)), k=k) for k, s in enumerate(stats)], thr,
                               bit_transition, max_dwells)
    assert (pos, n, int(rec["samplestamp"])) == (wpos, wn, want["k"] * 1000)
    # and the block itself, call by call, on grids whose outcome is given
    blk = qc.RefBlock(1000, 4, 2, 0, 250, max_dwells, thr, bit_transition, None,
                      grid=lambda s: dict(mag=float(np.float32(s)), input_power=1.0, acq_delay_samples=0.0, doppler_hz=0))
    blk.active = True
    blk.work([])  # state 0 -> 1
    calls = 0
    while blk.state == 1 and calls < len(stats):
        assert blk.work([stats[calls]]) == (1, 0)
        calls += 1
    assert (blk.state, calls) == ({True: 2, False: 3, None: 1}[pos], n)
    assert blk.sample_counter == calls * blk.L


def test_refblock_stamps_the_end_of_the_item_and_runs_the_state_machine():
    c = qc.quick_case("q4000x2")
    x = c.x.reshape(-1).astype(np.complex128)
    ref0 = c.reference(0, 0)["rec"]
    # positive at the first dwell
    blk = qc.RefBlock(c.fs, c.spc, c.p, c.dmax, c.dstep, 2, 0.5 * ref0["test_statistic"], False, c.codes[0])
    out = qc.run_attempts(blk, np.concatenate([x, x]), 1, per_call=2)[0]
    assert [(k["state"], k["consumed"], k["event"]) for k in out["calls"]] == [(0, 2, 0), (1, 1, 0), (2, 2, 1)]
    work = out["calls"][1]
    assert work["acq_samplestamp_samples"] == 2 * c.L + c.L  # two items skipped in state 0, then the end of the third
    assert (work["acq_delay_samples"], work["acq_doppler_hz"], work["acq_doppler_step"]) == \
        (c.reference(2, 0)["rec"]["acq_delay_samples"], float(c.reference(2, 0)["rec"]["doppler_hz"]), c.dstep)
    assert out["sample_counter"] == 5 * c.L and out["calls"][2]["acq_samplestamp_samples"] == 3 * c.L
    # the absent satellite: negative after max_dwells = 2; every dwell a grid of its own
    blk = qc.RefBlock(c.fs, c.spc, c.p, c.dmax, c.dstep, 2, 1e9, False, c.codes[3])
    blk.active = True
    blk.work([])  # state 0 -> 1 with nothing offered
    out = qc.run_attempts(blk, x, 1)[0]
    assert [(k["state"], k["event"]) for k in out["calls"]] == [(1, 0), (1, 0), (3, 2)]
    assert out["calls"][1]["test_statistic"] == pytest.approx(c.reference(1, 3)["rec"]["test_statistic"], rel=1e-12)
    assert out["calls"][1]["acq_samplestamp_samples"] == 2 * c.L


def test_adapter_defaults():
    assert [qc.default_folding_factor(s) for s in (2048, 4000, 8000, 25000)] == [4, 4, 4, 4]
    assert qc.default_folding_factor(1000) == 4 and qc.default_folding_factor(100000) == 5
    assert [qc.sampled_ms_key(v, 4) for v in (1, 4, 6, 8, 11)] == [4, 4, 4, 8, 8]


def test_struct_layout_matches_c_compiler(tmp_path):
    """The ctypes and numpy mirrors of gsdr_acq_quicksync_result vs sizeof / offsetof."""
    cname, py = "gsdr_acq_quicksync_result", gsdr.AcqQuickSyncResult
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsdr.h"', "int main(void){",
             'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for f, _ in py._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f))
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got[cname]) == ctypes.sizeof(py) == gsdr.ACQ_QUICKSYNC_RESULT_DTYPE.itemsize == 56
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset == gsdr.ACQ_QUICKSYNC_RESULT_DTYPE.fields[f][1], f

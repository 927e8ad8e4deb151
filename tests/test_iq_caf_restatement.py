"""The host-side pieces of the E5a IQ-CAF mode against the float64 restatement of
tests/iq_caf_checks.py: gsdr.iq_caf_decide against the restatement's block, the threshold formula, the
B-form construction, the window conditions, the periodic ties the comparisons allow for, and the
records' layout against the C compiler.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gsdr

import iq_caf_checks as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4000


def _records(rows):
    """rows: (mag, input_power, delay, doppler_hz, caf_doppler_hz) per dwell -> the device's records and
    the dicts the restatement's block is driven on."""
    out = np.zeros(len(rows), gsdr.ACQ_IQ_CAF_RESULT_DTYPE)
    dicts = []
    for k, (mag, ip, delay, dop, caf) in enumerate(rows):
        mag, ip = np.float32(mag), np.float32(ip)
        r = out[k]
        r["prn"], r["mag"], r["input_power"] = 11, mag, ip
        r["test_statistic"] = np.float32(mag / ip) if mag > 0 else 0.0
        r["acq_delay_samples"], r["doppler_hz"], r["caf_doppler_hz"] = delay, dop, caf
        r["doppler_index"], r["samplestamp"] = (dop + 1000) // 250, 500 + k * N
        dicts.append(dict(mag=float(mag), input_power=float(ip), acq_delay_samples=float(delay), doppler_hz=dop,
                          caf_doppler_hz=caf))
    return out, dicts


# (mag, input_power, delay, Doppler, CAF Doppler) per dwell.  STRONG_FIRST: the later dwell is weaker;
# WEAK_FIRST: the later one is stronger; EQUAL: the later one equals the statistic so far (strict '<');
# EMPTY_LAST: a dwell whose grid is all zeros has no winner.
STRONG_FIRST = [(0.30, 2.0, 17.0, 250, 0), (0.10, 2.0, 99.0, -500, -750), (0.20, 2.5, 5.0, 750, 500)]
WEAK_FIRST = [(0.02, 2.0, 17.0, 250, 0), (0.10, 2.0, 99.0, -500, -750), (0.30, 2.5, 5.0, 750, 500)]
EQUAL = [(0.25, 2.0, 17.0, 250, 0), (0.25, 2.0, 99.0, -500, -750)]
EMPTY_LAST = [(0.25, 2.0, 17.0, 250, 0), (0.0, 2.0, 0.0, 0, -1000)]
SEQUENCES = {"strong_first": STRONG_FIRST, "weak_first": WEAK_FIRST, "equal": EQUAL, "empty_last": EMPTY_LAST}


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("bit_transition", [False, True])
@pytest.mark.parametrize("caf", [False, True])
@pytest.mark.parametrize("max_dwells", [1, 2, 3])
def test_decide_against_the_block(seq, bit_transition, caf, max_dwells):
    recs, dicts = _records(SEQUENCES[seq])
    for thr in (0.04, 0.11, 0.2):
        syn, positive, dwells = gsdr.iq_caf_decide(recs, thr, bit_transition, max_dwells, caf_filter=caf)
        want, wpos, wdwells, wstat = qc.block_fold(dicts, N, float(np.float32(thr)), bit_transition, max_dwells, caf)
        assert (positive, dwells) == (wpos, wdwells), (seq, thr, syn, want)
        assert syn["acq_delay_samples"] == want["acq_delay_samples"]
        assert syn["acq_doppler_hz"] == want["acq_doppler_hz"]
        assert float(syn["test_statistics"]) == pytest.approx(wstat, rel=1e-6)
        # the record stamps the item's first sample from 500 on, the block the sample behind the item
        # from 0 on; no winner ever took over: both keep the zero of the restart
        if want["acq_samplestamp_samples"] == 0:
            assert syn["acq_samplestamp_samples"] == 0
        else:
            assert syn["acq_samplestamp_samples"] + N - 500 == want["acq_samplestamp_samples"]


def test_decide_cases_by_hand():
    recs, _ = _records(STRONG_FIRST)
    # without bit transition every dwell's winner takes over: the weaker second dwell decides
    syn, positive, dwells = gsdr.iq_caf_decide(recs, 0.11, False, 2)
    assert (positive, dwells, syn["acq_delay_samples"], syn["acq_doppler_hz"]) == (False, 2, 99.0, -500.0)
    # with it the first dwell's statistic stands, and its fields
    syn, positive, dwells = gsdr.iq_caf_decide(recs, 0.11, True, 2)
    assert (positive, dwells, syn["acq_delay_samples"], syn["acq_doppler_hz"]) == (True, 2, 17.0, 250.0)
    assert syn["acq_samplestamp_samples"] == 500
    # ... but the filter's Doppler of the second dwell overrides although its winner did not take over
    syn, positive, dwells = gsdr.iq_caf_decide(recs, 0.11, True, 2, caf_filter=True)
    assert (positive, syn["acq_delay_samples"], syn["acq_doppler_hz"]) == (True, 17.0, -750.0)
    # one dwell decides at once; fewer records than max_dwells decide nothing
    assert gsdr.iq_caf_decide(recs, 0.11, True, 1)[1:] == (True, 1)
    assert gsdr.iq_caf_decide(recs[:2], 0.11, True, 3)[1:] == (None, 2)
    # strict '<': an equal later dwell does not take over
    recs, _ = _records(EQUAL)
    assert gsdr.iq_caf_decide(recs, 0.11, True, 2)[0]["acq_delay_samples"] == 17.0
    assert gsdr.iq_caf_decide(recs, 0.11, False, 2)[0]["acq_delay_samples"] == 99.0
    # the decision is strict too
    assert gsdr.iq_caf_decide(recs, float(np.float32(0.125)), False, 2)[1] is False


def test_threshold_formula():
    for pfa, vlen, dmax, dstep in ((0.001, 32000, 5000, 250), (0.01, 64000, 10000, 250), (0.0001, 4000, 1000, 250)):
        t = gsdr.iq_caf_threshold(pfa, vlen, dmax, dstep)
        assert t == qc.threshold(pfa, vlen, dmax, dstep)
        bins = 2 * dmax // dstep + 1  # the inclusive count
        assert t == gsdr.tong_threshold(pfa, vlen, bins)
        # the quantile of the exponential distribution: 1 - exp(-lambda t) = (1 - pfa)^(1 / ncells)
        val = (1.0 - float(np.float32(pfa))) ** (1.0 / (vlen * bins))
        assert 1.0 - np.exp(-vlen * t) == pytest.approx(val, rel=1e-6)


def test_b_form():
    rng = np.random.default_rng(5)
    spc = 50
    for ms in (2, 3):
        a = qc.tiled(qc.random_code(rng, spc), ms, ms * spc)
        b = qc.b_form(a, spc)
        assert np.array_equal(b[:spc], -a[:spc]) and np.array_equal(b[spc:], a[spc:])
        fm = qc.forms(a, a, spc, ms, True)
        assert list(fm) == ["IA", "IB", "QA", "QB"]  # the engine's slot order
        assert np.array_equal(fm["QB"], b)
        # a period with its first sign flipped matches the B form in full and the A form in part
        s = a.copy()
        s[:spc] = -s[:spc]
        assert abs(np.vdot(b, s)) == ms * spc and abs(np.vdot(a, s)) == (ms - 2) * spc
    assert list(qc.forms(a, None, spc, 1, False)) == ["IA"]
    assert list(qc.forms(a, a, spc, 1, True)) == ["IA", "QA"]
    assert list(qc.forms(a, None, spc, 2, False)) == ["IA", "IB"]
    # zero padded: the period followed by zeros
    z = qc.tiled(qc.random_code(rng, spc), 1, 2 * spc)
    assert not z[spc:].any() and np.all(np.abs(z[:spc]) == 1.0)


def test_window_conditions():
    # CAF_bins_half = window / (2 step) in integers: 0 divides by zero at :605
    assert qc.window_error(499, 250, 21) and not qc.window_error(500, 250, 21)
    assert not qc.window_error(0, 250, 21) and not qc.window_error(-5, 250, 21)
    # the body loop's window of 2 half + 1 rows must fit the grid
    assert not qc.window_error(5000, 250, 21) and qc.window_error(5500, 250, 21)   # half 10 / 11
    assert not qc.window_error(2000, 250, 9) and qc.window_error(2500, 250, 9)     # half 4 / 5
    # at the largest window every loop index stays inside the vectors
    for D, half in ((21, 10), (9, 4), (3, 1)):
        caf = qc.caf_vector(list(range(1, D + 1)), list(range(D, 0, -1)), 250, 500 * half, True)
        assert len(caf) == D and all(np.isfinite(caf))


def test_caf_vector_by_hand():
    # half = 1, w = 0.5, one component, peaks (1, 2, 4): the signed weight of :614 and :634 is
    # 1 - 0.5 (d - i): 1.5 for the row above, 0.5 for the row below; the last loop has abs
    caf = qc.caf_vector([1.0, 2.0, 4.0], [0.0] * 3, 250, 500, False)
    assert caf[0] == pytest.approx((1.0 * 1.0 + 2.0 * 1.5) / (1.0 + 1.0 - 0.5 * 1.0 * (2.0 / 2.0) - 0.0))
    assert caf[1] == pytest.approx((1.0 * 0.5 + 2.0 + 4.0 * 1.5) / (1.0 + 2.0 - 2.0 * 0.5 * 1.0 * 2.0 / 2.0))
    assert caf[2] == pytest.approx((2.0 * 0.5 + 4.0) / (1.0 + 1.0 + 0.0 - 0.5 * 1.0 * 2.0 / 2.0 - 0.0))
    # both components: Q has abs in the first loop and the signed weight in the body
    caf = qc.caf_vector([0.0] * 3, [1.0, 2.0, 4.0], 250, 500, True)
    assert caf[0] == pytest.approx((1.0 + 2.0 * 0.5) / 1.5)
    assert caf[1] == pytest.approx((1.0 * 0.5 + 2.0 + 4.0 * 1.5) / 2.0)


@pytest.mark.parametrize("name", ["q2000", "q3000"])
def test_periodic_ties(name):
    """An A form's row repeats every samples_per_code (so does the 2 ms B form's): the restatement's
    winner has equals spc apart, is not `pinned`, and only the delay is compared.  A row chosen from a
    3 ms B form, or one period over a one-period item, is pinned.  (The zero-padded replica sees other
    noise a period later: its two peaks differ, and the margin says whether by enough.)"""
    c = qc.iq_caf_case(name)
    x = c.x[0].astype(np.complex128)
    fm = c.fm[0]
    cf = {k: np.conj(np.fft.fft(v)) for k, v in fm.items()}
    X = np.fft.fft(x * qc.wipeoff(c.rows[c.truth[0]["row"]], c.fs, c.n))
    for k in fm:
        r = np.fft.ifft(X * cf[k]) * c.n
        mag = r.real ** 2 + r.imag ** 2
        periodic = k[1] == "A" or c.n // c.spc == 2
        if periodic and c.n > c.spc:
            assert np.allclose(mag, np.roll(mag, c.spc), rtol=1e-9, atol=1e-9 * mag.max()), (name, k)
    rec, rr = c.reference(c.windows[0])[0][0]
    assert not rec["pinned"] and not rr[c.truth[0]["row"]]["pinned"]
    if name == "q3000":
        k = [t["scenario"] for t in c.truth].index("BB")
        assert c.reference(c.windows[0])[k][0][0]["pinned"]
    one = qc.iq_caf_case("p8000")
    assert one.reference(one.windows[0])[0][0][0]["pinned"]


def test_record_layouts_match_c_compiler(tmp_path):
    src = tmp_path / "iq_caf_layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsdr.h"', "int main(void){"]
    for st, cls in (("gsdr_acq_iq_caf_row", gsdr.AcqIqCafRow), ("gsdr_acq_iq_caf_result", gsdr.AcqIqCafResult)):
        lines.append('printf("%s.size %%zu\\n", sizeof(%s));' % (st, st))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (st, f, st, f))
    lines.append("return 0;}")
    src.write_text("\n".join(lines))
    exe = tmp_path / "iq_caf_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for st, cls, dt, size in (("gsdr_acq_iq_caf_row", gsdr.AcqIqCafRow, gsdr.ACQ_IQ_CAF_ROW_DTYPE, 24),
                              ("gsdr_acq_iq_caf_result", gsdr.AcqIqCafResult, gsdr.ACQ_IQ_CAF_RESULT_DTYPE, 56)):
        assert int(got[st + ".size"]) == ctypes.sizeof(cls) == dt.itemsize == size
        assert [f for f, _ in cls._fields_] == list(dt.names)
        for f, _ in cls._fields_:
            assert int(got["%s.%s" % (st, f)]) == getattr(cls, f).offset == dt.fields[f][1], (st, f)


def test_entry_points_are_declared_and_bound():
    txt = open(os.path.join(ROOT, "include", "gsdr.h")).read()
    names = {"gsdr_acq_set_iq_caf", "gsdr_acq_set_iq_codes", "gsdr_acq_run_iq_caf", "gsdr_acq_run_iq_caf_stream",
             "gsdr_acq_dump_iq_caf_rows"}
    assert names <= set(re.findall(r"\b(gsdr_[a-z0-9_]+)\s*\(", txt))
    assert names <= set(gsdr.EXPORTED)
    L = gsdr.load()
    assert L.gsdr_abi_version() == 1  # entry points were added; no layout or signature changed
    assert L.gsdr_acq_set_iq_caf(None, 1000, 1, 0, 0) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_set_iq_codes(None, None, None, None, 0) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_iq_caf(None, None, 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_iq_caf_stream(None, None, 0, 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_iq_caf_rows(None, None, None) == gsdr.GSDR_E_ARG


def test_every_case_meets_its_margins():
    """The restatement alone: every margin the GPU comparisons rest on, and what each scenario is there
    to show (the small cases; the GPU tests assert the same for every case before they compare)."""
    for name in ("q2000", "q3000", "q4000", "z4000", "f2000"):
        c = qc.iq_caf_case(name)
        for w in c.windows:
            qc.assert_margins(c, w)
        qc.expectations(c)
        assert qc.seed_search(name, qc.SEED_OFFSETS.get(name, 0) + 1) == qc.SEED_OFFSETS.get(name, 0)

"""The fine-Doppler restatement (tests/fine_checks.py) and the new ABI structs, no GPU: the
eight-residue identity the device kernel computes by, the reference's replica alignment
with its quirk, the frequency formula's arithmetic, the shared inputs' distance from a
near tie, and the struct layouts against the C compiler."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gsdr
from gsdr import synth

import fine_checks as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_eight_residue_identity(name):
    """X[8 q + r] = FFT_L(y e^{-2 pi i n r / M})[q] against numpy's FFT of the padded
    buffer: every bin within 1e-12 of the maximum, the same first maximum."""
    c = fc.fine_case(name)
    shift, _, slot = c.requests[0]
    y = fc.wiped(c.x, c.codes[slot], shift)
    X, Xr = fc.padded_spectrum(y), fc.residue_spectrum(y)
    assert len(X) == len(Xr) == 80 * c.N
    assert np.max(np.abs(X - Xr)) <= 1e-12 * np.max(np.abs(X))
    assert int(np.argmax(np.abs(X) ** 2)) == int(np.argmax(np.abs(Xr) ** 2)) == c.reference(0)["index"]


@pytest.mark.parametrize("n", [8, 2000])
def test_rotate_quirk(n):
    """std::rotate(c, c + (N - shift), c + N - 1): the last sample never moves; shift 0 and
    1 leave the row alone; shift >= 2 gives c'[i] = c[(i + N - shift) mod (N - 1)], i < N - 1."""
    c = np.arange(n) + 100
    for shift in (0, 1):
        assert np.array_equal(fc.rotate_replica(c, shift), c)
    for shift in (2, n // 2, n - 1):
        r = fc.rotate_replica(c, shift)
        assert r[n - 1] == c[n - 1]
        i = np.arange(n - 1)
        assert np.array_equal(r[:n - 1], c[(i + n - shift) % (n - 1)])
    # shift 2 moves the first N - 1 samples by one place, shift N - 1 brings c[1] to the front
    assert np.array_equal(fc.rotate_replica(c, 2)[:3], [c[n - 2], c[0], c[1]])
    assert np.array_equal(fc.rotate_replica(c, n - 1)[:2], [c[1], c[2]])
    assert fc.rotate_replica(c, n - 1)[n - 2] == c[0]


@pytest.mark.parametrize("fs,N", [(2000000, 2000), (2048000, 2048), (4000000, 4000), (25000000, 25000)])
def test_frequency_formula(fs, N):
    """fftFreqBins at k = 0, M/2 - 1, M/2, M - 1: float operands, double product and quotient,
    one rounding (the reference's 2.0 literals are doubles)."""
    M = 80 * N
    step = fs / M
    assert fc.freq_bin(0, fs, M) == np.float32(0.0)
    assert fc.freq_bin(M // 2 - 1, fs, M) == np.float32(step * (M // 2 - 1))
    assert fc.freq_bin(M // 2, fs, M) == np.float32(-fs / 2.0)
    assert fc.freq_bin(M - 1, fs, M) == np.float32(-step)
    assert fc.freq_bin(M // 2 - 1, fs, M).dtype == np.float32


def test_frequency_formula_is_the_double_one():
    """Where the two readings of :394-404 differ: with every operation rounded to float the
    product (fs / 2) k rounds before the division, e.g. 25 Msps bin 43 gives 537.50006 and
    4 Msps bin 1075 gives 13437.501; the reference's doubles give 537.5 and 13437.5."""
    f32 = np.float32

    def all_float(k, fs, M):
        return f32(f32(f32(f32(fs) / f32(2)) * f32(k)) / f32(f32(M) / f32(2)))

    for fs, N, k, want in ((25000000, 25000, 43, 537.5), (4000000, 4000, 1075, 13437.5), (2000000, 2000, 1077, 13462.5)):
        M = 80 * N
        assert fc.freq_bin(k, fs, M) == f32(want) == f32(k * fs / M)
        assert all_float(k, fs, M) != f32(want)
    # the 25 Msps case of the GPU tests has its peaks at such bins
    c = fc.fine_case("four250000")
    assert [all_float(k, c.fs, c.M) != fc.freq_bin(k, c.fs, c.M) for k in (43, 45)] == [True, True]
    assert c.reference(0)["index"] == 43 and c.reference(1)["index"] == c.M - 45


def test_shared_inputs_are_far_from_a_tie():
    """Every request of every case: the restatement's best bin is MIN_MARGIN above its second
    best; the satellites are found at their bins; the peaks cover every residue mod 8, both
    signs of the frequency, and the code phases 0, 1, 2, N - 1."""
    residues, phases, negative = set(), set(), 0
    for name in sorted(fc.CASES):
        c = fc.fine_case(name)
        assert c.x.dtype == np.complex64 and len(c.x) == 10 * c.N
        for i in range(4):
            r = c.reference(i)
            assert r["margin"] >= fc.MIN_MARGIN, (name, i, r["margin"])
            if i < 3:
                assert r["index"] == c.true_index[i] and r["accepted"] == 1, (name, i, r["index"])
                assert r["doppler_hz"] == fc.CASES[name]["sats"][i][1] * 12.5
                residues.add(r["index"] % 8)
                negative += r["index"] >= c.M // 2
                phases.add(c.requests[i][0] if c.requests[i][0] < 3 else c.requests[i][0] - c.N)
    assert residues == set(range(8))
    assert negative >= 2
    assert {0, 1, 2, -1} <= phases


def test_item_type_inputs_are_far_from_a_tie():
    c = fc.fine_case("four40000")
    for it in (gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE):
        raw, z = c.items(it)
        assert raw.dtype == (np.int16 if it == gsdr.ITEM_CSHORT else np.int8) and len(z) == c.L
        for i in range(4):
            assert c.reference(i, it)["margin"] >= fc.MIN_MARGIN


def test_rejected_estimate():
    """A coarse Doppler 1250 Hz off the fine one is kept (:412-416)."""
    c = fc.fine_case("lds20000")
    true = c.reference(0)["doppler_hz"]
    r = c.reference(0, 0, true + 1250.0)
    assert r["accepted"] == 0 and r["doppler_hz"] == true + 1250.0 and float(r["freq_hz"]) == true


def test_fine_struct_layouts_match_c_compiler(tmp_path):
    """ctypes and numpy mirrors of gsdr_acq_fine_request / gsdr_acq_fine_result vs the C
    compiler's sizeof / offsetof."""
    pairs = (("gsdr_acq_fine_request", gsdr.AcqFineRequest, gsdr.ACQ_FINE_REQUEST_DTYPE),
             ("gsdr_acq_fine_result", gsdr.AcqFineResult, gsdr.ACQ_FINE_RESULT_DTYPE))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsdr.h"', "int main(void){"]
    for cname, py, _ in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _t in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0;}")
    src = tmp_path / "fine_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "fine_layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, py, dt in pairs:
        assert int(got[cname]) == ctypes.sizeof(py) == dt.itemsize, cname
        assert [f for f, _t in py._fields_] == list(dt.names)
        for f, _t in py._fields_:
            assert int(got[cname + "." + f]) == getattr(py, f).offset == dt.fields[f][1], (cname, f)


def test_fine_entry_points_reject_null():
    L = gsdr.load()
    assert L.gsdr_acq_fine_doppler(None, None, None, 0, None, 0, None) == gsdr.GSDR_E_ARG
    assert b"null" in L.gsdr_last_error()
    assert L.gsdr_acq_fine_doppler_stream(None, None, 0, None, 0, None, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_fine_spectrum(None, None, None, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_get_fine_plan(None, None, None, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_get_fine_ready(None, None) == gsdr.GSDR_E_ARG


def test_replica_of_the_inputs_is_the_acquisition_replica():
    c = fc.fine_case("lds20000")
    assert np.array_equal(c.codes[0], synth.gps_ca_sampled(c.prns[0], c.fs))

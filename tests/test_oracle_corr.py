"""The oracle's exact multicorrelator companions and the integer probe's own
helpers, on the CPU alone (tests/corr_checks.py states the probe).

- multicorrelator_complex_codes_exact / multicorrelator_real_codes_hd_exact agree
  with the reference restatements they accompany to 1e-4 (the project's bound for
  the reference's fp32 kernels) on strong-signal inputs, and reduce to
  multicorrelator_real_codes_exact where the operations coincide.
- The probe's int64 sums are what multicorrelator_real_codes_exact computes, and
  the parameters of the generic / a_avx cases do separate the two associations.
"""
import numpy as np
import pytest

from gsdr import synth
from oracle import volk

import corr_checks as cc
from conftest import vnorm_rel


@pytest.mark.parametrize("doppler", [800.0, -800.0])
def test_complex_exact_agrees_with_reference(doppler):
    fs, N = 4e6, 8197
    code = cc.complex_code(9)
    x = cc.strong_signal(fs, N, 9, doppler, seed=3)
    args = (0.7, cc.f32(2 * np.pi * doppler / fs), 0.05, cc.f32(1.023e6 / fs))
    ref = volk.multicorrelator_complex_codes(x, code, cc.SHIFTS5, *args, N)
    exact = volk.multicorrelator_complex_codes_exact(x, code, cc.SHIFTS5, *args, N)
    err = vnorm_rel(ref, exact)
    print("complex codes, doppler %+.0f: reference vs exact %.2e" % (doppler, err))
    assert err <= 1e-4


@pytest.mark.parametrize("N", [4000, 4396])
def test_hd_exact_agrees_with_reference(N):
    fs = 4e6
    code = synth.gps_ca_chips(11)
    x = cc.strong_signal(fs, N, 11, 2100.0, seed=4)
    kw = dict(carr_rate=2e-9, code_rate=1e-10)
    args = (0.1, cc.f32(2 * np.pi * 2100.0 / fs), 0.05, cc.f32(1.023e6 / fs))
    ref = volk.multicorrelator_real_codes(x, code, cc.SHIFTS5, *args, N, high_dyn=True, **kw)
    exact = volk.multicorrelator_real_codes_hd_exact(x, code, cc.SHIFTS5, *args, N, **kw)
    err = vnorm_rel(ref, exact)
    print("high dynamics N=%d: reference vs exact %.2e" % (N, err))
    assert err <= 1e-4


def test_complex_exact_reduces_to_real_exact():
    fs, N = 4e6, 8197
    code = synth.gps_ca_chips(9)
    x = cc.strong_signal(fs, N, 9, 800.0, seed=3)
    for assoc in (cc.GENERIC, cc.AVX):
        args = (0.7, cc.f32(2 * np.pi * 800.0 / fs), cc.AG_REM, cc.AG_STEP)
        real = volk.multicorrelator_real_codes_exact(x, code, cc.AG_SHIFTS, *args, N, assoc=assoc)
        cplx = volk.multicorrelator_complex_codes_exact(x, code.astype(np.complex64), cc.AG_SHIFTS, *args, N,
                                                        assoc=assoc)
        np.testing.assert_array_equal(cplx, real)


def test_hd_exact_reduces_to_real_exact():
    """Rates 0 and one tap: the high-dynamics index is the generic association's and
    the rate phasor is (1, 0)."""
    fs, N = 4e6, 4396
    code = synth.gps_ca_chips(11)
    x = cc.strong_signal(fs, N, 11, 2100.0, seed=4)
    args = (0.1, cc.f32(2 * np.pi * 2100.0 / fs), cc.AG_REM, cc.AG_STEP)
    for shift in (0.0, 0.15):
        real = volk.multicorrelator_real_codes_exact(x, code, [shift], *args, N, assoc=cc.GENERIC)
        hd = volk.multicorrelator_real_codes_hd_exact(x, code, [shift], *args, N)
        np.testing.assert_array_equal(hd, real)


def test_hd_exact_rate_terms_are_live():
    """The rate arguments reach the result (a dropped argument would pass the reductions)."""
    fs, N = 4e6, 4396
    code = synth.gps_ca_chips(11)
    x = cc.strong_signal(fs, N, 11, 2100.0, seed=4)
    args = (0.1, cc.f32(2 * np.pi * 2100.0 / fs), 0.05, cc.f32(1.023e6 / fs))
    hd = volk.multicorrelator_real_codes_hd_exact
    base = hd(x, code, cc.SHIFTS5, *args, N)
    assert vnorm_rel(hd(x, code, cc.SHIFTS5, *args, N, carr_rate=2e-7), base) > 1e-2
    assert vnorm_rel(hd(x, code, cc.SHIFTS5, *args, N, code_rate=2e-8), base) > 1e-3


def test_probe_expected_is_the_exact_oracle():
    N = 8197
    iq = cc.probe_iq(N, 1)
    x = cc.iq_items(iq)
    for cplx, exact in ((False, volk.multicorrelator_real_codes_exact),
                        (True, volk.multicorrelator_complex_codes_exact)):
        ch = cc.Chan(cc.probe_code(cc.AG_L, 1, cplx), cc.AG_SHIFTS)
        for assoc in (cc.GENERIC, cc.AVX):
            want = exact(x, ch.code, ch.shifts, 0.0, 0.0, cc.AG_REM, cc.AG_STEP, N, assoc=assoc)
            got = cc.expected(iq, ch, cc.indices(ch, cc.AG_REM, cc.AG_STEP, N, assoc=assoc))
            np.testing.assert_array_equal(got.astype(np.complex128), want)
    hd = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS, high_dyn=True)
    want = volk.multicorrelator_real_codes_hd_exact(x[:4396], hd.code, hd.shifts, 0.0, 0.0, cc.AG_REM, cc.AG_STEP,
                                                    4396, code_rate=2e-8)
    got = cc.expected(iq[:4396], hd, cc.indices(hd, cc.AG_REM, cc.AG_STEP, 4396, rate=2e-8))
    np.testing.assert_array_equal(got.astype(np.complex128), want)


@pytest.mark.parametrize("N", [4000, 8197])
def test_probe_parameters_separate_the_associations(N):
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS)
    e = cc.expected_both_assocs(cc.probe_iq(N, 1), ch, cc.AG_REM, cc.AG_STEP, N)
    assert np.any(e[cc.GENERIC] != e[cc.AVX])
    # and the dyadic shifts of the tap tests do not: the probe needs its own
    dy = cc.Chan(ch.code, [-0.5, -0.25, 0.0, 0.25, 0.5])
    assert np.array_equal(cc.indices(dy, cc.AG_REM, cc.AG_STEP, N, cc.GENERIC),
                          cc.indices(dy, cc.AG_REM, cc.AG_STEP, N, cc.AVX))


def test_probe_raw_index_model_and_spans():
    """raw_indices (numpy float32) wraps to the oracle's index, and the shapes of the
    span cases land where test_gpu_corr_paths.py says they do."""
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS)
    for assoc in (cc.GENERIC, cc.AVX):
        for step in (cc.AG_STEP, -cc.AG_STEP, 0.0, 1.0):
            raw = cc.raw_indices(ch, cc.AG_REM, step, np.arange(8197), assoc)
            np.testing.assert_array_equal(raw % ch.L, cc.indices(ch, cc.AG_REM, step, 8197, assoc=assoc))
    assert cc.chunk_spans(ch, cc.AG_REM, cc.AG_STEP, 4000) == [1025]
    spans = cc.chunk_spans(ch, cc.AG_REM, cc.AG_STEP, 8197)
    assert len(spans) == 3 and spans[0] > ch.L and spans[1] > ch.L and spans[2] <= 3
    code = cc.probe_code(1023, 3)
    assert cc.chunk_spans(cc.Chan(code, [0.0]), 0.0, 1.0, 4096) == [cc.SPAN_CAP]
    assert cc.chunk_spans(cc.Chan(code, [0.0, 1.0]), 0.0, 1.0, 4096) == [cc.SPAN_CAP + 1]
    b1i = cc.Chan(cc.probe_code(2046, 4), [-0.5, 0.0, 0.5])
    assert cc.chunk_spans(b1i, 0.0, cc.f32(2.046e6 / 2e6), 4196) == [4191, 103]


def test_probe_window_zero_pads():
    iq = cc.probe_iq(100, 2)
    w = cc.window(iq, -10, 30)
    assert not w[:10].any() and np.array_equal(w[10:], iq[:20])
    w = cc.window(iq, 90, 30)
    assert np.array_equal(w[:10], iq[90:]) and not w[10:].any()
    assert not cc.window(iq, 100, 5).any() and cc.window(iq, 3, 0).shape == (0, 2)


def test_probe_refuses_inexact_inputs():
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), [0.0])
    with pytest.raises(AssertionError):
        cc.expected(cc.probe_iq(4000, 1) * 40, ch, cc.indices(ch, 0.0, cc.AG_STEP, 4000))
    half = cc.Chan(ch.code + 0.5, [0.0])
    with pytest.raises(AssertionError):
        cc.expected(cc.probe_iq(100, 1), half, cc.indices(half, 0.0, cc.AG_STEP, 100))

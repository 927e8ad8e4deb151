"""Acquisition resampler design (no GPU): gsdr_acq_resampler_plan restates
Acq_Conf::ConfigureAutomaticResampler (acq_conf.cc:97-106) and the flowgraph's
filter design (gnss_flowgraph.cc:1073-1087,1112); gsdr_firdes_low_pass restates
firdes::low_pass with the Hamming window."""
import numpy as np
import pytest

import gsdr


def low_pass_ref(gain, fs, cutoff, tw):
    """The definition in include/gsdr.h, restated in numpy (taps and window stored as float32)."""
    ntaps = int(53.0 * fs / (22.0 * tw))
    if ntaps % 2 == 0:
        ntaps += 1
    M = (ntaps - 1) // 2
    w = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(ntaps) / (ntaps - 1))).astype(np.float32)
    om = 2.0 * np.pi * cutoff / fs
    taps = np.zeros(ntaps, np.float32)
    for n in range(-M, M + 1):
        c = om / np.pi if n == 0 else np.sin(n * om) / (n * np.pi)
        taps[n + M] = np.float32(c * float(w[n + M]))
    fmax = float(taps[M]) + 2.0 * float(np.sum(taps[M + 1:].astype(np.float64)))
    return (taps.astype(np.float64) * (gain / fmax)).astype(np.float32)


@pytest.mark.parametrize("fs,opt,want", [
    (4e6, 2e6, (2, 9, 4)), (8e6, 2e6, (4, 19, 9)), (16e6, 2e6, (8, 39, 19)), (25e6, 2e6, (10, 49, 24))])
def test_plan_values(fs, opt, want):
    assert gsdr.acq_resampler_plan(fs, opt) == want


def test_plan_other_optimum_and_no_resampler():
    assert gsdr.acq_resampler_plan(25e6, 1e7)[0] == 2
    # fs <= opt, and floor(3/2) = 1: no resampler
    assert gsdr.acq_resampler_plan(2e6, 2e6) == (1, 0, 0)
    assert gsdr.acq_resampler_plan(3e6, 2e6) == (1, 0, 0)
    # 6.625 Msps: floor(3.3) = 3 does not divide the rate, 2 does
    assert gsdr.acq_resampler_plan(6625000, 2e6)[0] == 2
    for bad in ((0, 2e6), (4e6, 0.0)):
        with pytest.raises(gsdr.GsdrError) as e:
            gsdr.acq_resampler_plan(*bad)
        assert e.value.code == gsdr.GSDR_E_ARG


@pytest.mark.parametrize("fs,opt", [(4e6, 2e6), (8e6, 2e6), (16e6, 2e6), (25e6, 2e6), (25e6, 1e7), (12.5e6, 4e6)])
def test_low_pass_matches_restatement(fs, opt):
    d, ntaps, lat = gsdr.acq_resampler_plan(fs, opt)
    fs_d = fs / d
    got = gsdr.firdes_low_pass(1.0, fs, fs_d / 2.1, fs_d / 2.0)
    ref = low_pass_ref(1.0, fs, fs_d / 2.1, fs_d / 2.0)
    assert got.dtype == np.float32 and len(got) == ntaps == len(ref) and lat == (ntaps - 1) // 2
    assert np.max(np.abs(got.astype(np.float64) - ref)) <= 2e-7
    np.testing.assert_array_equal(got, got[::-1])  # symmetric
    assert abs(float(np.sum(got.astype(np.float64))) - 1.0) <= 1e-6


def test_low_pass_gain_scales():
    a = gsdr.firdes_low_pass(1.0, 4e6, 2e6 / 2.1, 1e6)
    b = gsdr.firdes_low_pass(2.5, 4e6, 2e6 / 2.1, 1e6)
    assert abs(float(np.sum(b.astype(np.float64))) - 2.5) <= 2.5e-6
    assert np.max(np.abs(b - 2.5 * a)) <= 2e-7


def test_low_pass_pinned_taps():
    """The 9 taps of the 4 Msps -> 2 Msps resampler.  The pinned values come from the
    numpy restatement above (the formula in include/gsdr.h); GNU Radio itself was not
    available to pin them further."""
    half = np.array([-0.00187097, -0.02214734, 0.01277171, 0.27384892, 0.47479537])
    want = np.concatenate([half, half[-2::-1]])
    got = gsdr.firdes_low_pass(1.0, 4e6, 2e6 / 2.1, 1e6)
    assert len(got) == 9
    assert np.max(np.abs(got.astype(np.float64) - want)) <= 1e-7


def test_low_pass_rejects_bad_arguments():
    for args in ((1.0, 4e6, 0.0, 1e6), (1.0, 4e6, 2.1e6, 1e6), (1.0, 4e6, 1e6, 0.0), (1.0, 4e6, 1e6, -1.0)):
        with pytest.raises(gsdr.GsdrError) as e:
            gsdr.firdes_low_pass(*args)
        assert e.value.code == gsdr.GSDR_E_ARG
    # a buffer shorter than the design
    L = gsdr.load()
    import ctypes
    taps = np.zeros(4, np.float32)
    n = ctypes.c_uint32(4)
    rc = L.gsdr_firdes_low_pass(1.0, 4e6, 2e6 / 2.1, 1e6, ctypes.c_void_p(taps.ctypes.data), ctypes.byref(n))
    assert rc == gsdr.GSDR_E_ARG

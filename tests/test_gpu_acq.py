"""GPU parity of the PCPS acquisition engine against the oracle (pcps_acquisition
restatement), through the C ABI.

Tolerances (BASELINE.json north_star): CAF peak, input power, second peak and test
statistic within 1e-4 relative (fp32); Doppler index and code phase equal, or — the
near-tie rule of SURVEY §7 H3 — the oracle's grid value at the GPU's cell within
1e-4 of the oracle's maximum.
"""
import json
import os

import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import pcps, replica

from acq_checks import RTOL, _check_result, _codes, _oracle_grids  # noqa: F401 (other test modules import them from here)

pytestmark = pytest.mark.gpu


def test_reference_capture_validation(gps_capture):
    """The reference's ValidationOfResults case on its own capture, via the GPU."""
    fs, dmax, dstep = 4000000, 5000, 100
    acq = gsdr.Acquisition(fs, 4000, dmax, dstep, pfa=0.0, max_prns=1)
    assert acq.num_doppler_bins == 100 and acq.fft_size == 4000
    acq.set_local_codes(replica.gps_l1_ca_code_complex_sampled(1, fs)[None, :], [1])
    acq.set_threshold(0.001)
    r = acq.run(gps_capture[:4000])[0, 0]
    assert r["prn"] == 1 and r["positive"] == 1
    assert abs(524 - r["acq_delay_samples"]) * 1023 / 4000 < 0.5
    assert abs(1680 - r["doppler_hz"]) <= 666
    M = _oracle_grids(gps_capture[:4000], [replica.gps_l1_ca_code_complex_sampled(1, fs)], fs, dmax, dstep, 100)[0]
    assert _check_result(r, M, 0.0, 4, fs, dmax, dstep, 4000.0)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("D", [80, 81])
def test_c2_synthetic_32prn(pfa, D):
    """Config C2: 4 Msps, 32 PRNs x D Doppler bins (+-10 kHz, 250 Hz), 8 visible."""
    fs, N, dmax, dstep = 4000000, 4000, 10000, 250
    sats = synth.random_constellation(8, seed_offset=2)
    x = synth.gps_l1_iq(fs, N, sats, seed_offset=2)
    prns = np.arange(1, 33)
    codes = _codes(prns, fs, N)
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=pfa, max_prns=32, num_doppler_bins=D)
    acq.set_local_codes(codes, prns)
    if pfa > 0:
        assert abs(acq.threshold - pcps.threshold(pfa, N, D)) <= 1e-6 * pcps.threshold(pfa, N, D)
    res = acq.run(x)[0]
    grids = _oracle_grids(x, codes, fs, dmax, dstep, D)
    exact = 0
    for p in range(32):
        exact += _check_result(res[p], grids[p], pfa, 4, fs, dmax, dstep, 4000.0)
        assert res[p]["prn"] == prns[p]
    # cells equal to the oracle's vs H3 near ties (the oracle's grid value at the
    # GPU's cell within 1e-4 of its maximum), logged for the record
    line = {"tag": "c2_acq", "pfa": pfa, "D": D, "prns": 32, "exact_cells": int(exact), "near_ties": int(32 - exact)}
    print("parity acq", json.dumps(line))
    if os.environ.get("GSDR_PARITY_LOG"):
        with open(os.environ["GSDR_PARITY_LOG"], "a") as f:
            f.write(json.dumps(line) + "\n")
    assert exact >= 30
    visible = {s.prn for s in sats}
    if pfa > 0:
        detected = {int(r["prn"]) for r in res if r["positive"]}
        # 45 dB-Hz in 1 ms with up to 125 Hz Doppler mismatch: most, not all, cross the threshold
        assert len(visible & detected) >= 6
        for p in range(32):
            ti, di, gmax, ip, stat = pcps.max_to_input_power_statistic(grids[p])
            if abs(stat - acq.threshold) > 1e-3 * acq.threshold:
                assert bool(res[p]["positive"]) == bool(stat > acq.threshold)


def test_multiblock_and_stamps():
    fs, N, dmax, dstep = 4000000, 4000, 10000, 250
    sats = synth.random_constellation(8, seed_offset=5)
    nb = 4
    x = synth.gps_l1_iq(fs, N * nb, sats, seed_offset=5)
    prns = np.array([s.prn for s in sats] + [33 - s.prn for s in sats[:2]])
    codes = _codes(prns, fs, N)
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.01, max_prns=len(prns), max_blocks=nb)
    acq.set_local_codes(codes, prns)
    res = acq.run(x, nblocks=nb, stamp0=12345)
    for b in range(nb):
        xb = x[b * N:(b + 1) * N]
        grids = _oracle_grids(xb, codes, fs, dmax, dstep, 80)
        for p in range(len(prns)):
            _check_result(res[b, p], grids[p], 0.01, 4, fs, dmax, dstep, 4000.0)
            assert res[b, p]["samplestamp"] == 12345 + b * N


@pytest.mark.parametrize("fs", [2000000, 8000000, 16000000, 6000000])
def test_other_sample_rates(fs):
    """Static plans for 2/8/16 Msps and the runtime-planned fallback (6 Msps: N=6000)."""
    N = fs // 1000
    dmax, dstep = 5000, 500
    sats = synth.random_constellation(4, seed_offset=fs // 1000000)
    x = synth.gps_l1_iq(fs, N, sats, seed_offset=3)
    prns = np.array([s.prn for s in sats][:3])
    codes = _codes(prns, fs, N)
    spc = int(np.ceil(fs / 1023000.0))
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.0, max_prns=3)
    acq.set_local_codes(codes, prns)
    res = acq.run(x)[0]
    grids = _oracle_grids(x, codes, fs, dmax, dstep, 20)
    for p in range(3):
        _check_result(res[p], grids[p], 0.0, spc, fs, dmax, dstep, float(np.float32(fs) * np.float32(0.001)))


def test_grid_dump_matches_oracle_grid():
    fs, N, dmax, dstep = 4000000, 4000, 10000, 250
    sats = synth.random_constellation(8, seed_offset=9)
    x = synth.gps_l1_iq(fs, N, sats, seed_offset=9)
    prns = np.array([sats[0].prn, sats[1].prn])
    codes = _codes(prns, fs, N)
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.01, max_prns=2)
    acq.set_local_codes(codes, prns)
    g = acq.dump_grid(x, 1)
    M = _oracle_grids(x, codes[1:2], fs, dmax, dstep, 80)[0]
    assert np.max(np.abs(g - M)) <= 1e-5 * M.max()


def test_forward_spectra_match_numpy():
    fs, N, dmax, dstep = 4000000, 4000, 10000, 250
    x = synth.gps_l1_iq(fs, N, synth.random_constellation(4, seed_offset=11), seed_offset=11)
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.01, max_prns=1)
    acq.set_local_codes(_codes([1], fs, N), [1])
    X = acq.dump_spectra(x)
    wipe = pcps.doppler_wipeoffs(fs, N, dmax, dstep, 80)
    ref = np.fft.fft(x.astype(np.complex128)[None, :] * wipe.astype(np.complex128), axis=1)
    err = np.abs(X - ref).max() / np.abs(ref).max()
    assert err < 2e-6


def test_cshort_input():
    fs, N, dmax, dstep = 4000000, 4000, 10000, 250
    sats = synth.random_constellation(8, seed_offset=13)
    x = synth.gps_l1_iq(fs, N, sats, seed_offset=13)
    xs = synth.to_cshort(x, 2000.0)
    xf = (xs[0::2].astype(np.float32) + 1j * xs[1::2].astype(np.float32)).astype(np.complex64)
    prns = np.array([s.prn for s in sats[:4]])
    codes = _codes(prns, fs, N)
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.01, max_prns=4, item_type=gsdr.ITEM_CSHORT)
    acq.set_local_codes(codes, prns)
    res = acq.run(xs)[0]
    grids = _oracle_grids(xf, codes, fs, dmax, dstep, 80)
    for p in range(4):
        _check_result(res[p], grids[p], 0.01, 4, fs, dmax, dstep, 4000.0)


def test_ibyte_input():
    """SignalSource.item_type=byte through Ibyte_To_Complex: the engine reads the
    interleaved int8 pairs directly (exact conversion), identical to gr_complex input
    of the converted samples."""
    fs, N, dmax, dstep = 4000000, 4000, 10000, 250
    sats = synth.random_constellation(8, seed_offset=17, cn0_dbhz=50.0)
    x = synth.gps_l1_iq(fs, N, sats, seed_offset=17)
    xb = synth.to_ibyte(x, 24.0)
    xf = synth.ibyte_to_complex(xb)
    prns = np.array([s.prn for s in sats[:4]])
    codes = _codes(prns, fs, N)
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.01, max_prns=4, item_type=gsdr.ITEM_IBYTE)
    acq.set_local_codes(codes, prns)
    res = acq.run(xb)[0]
    ref = gsdr.Acquisition(fs, N, dmax, dstep, pfa=0.01, max_prns=4)
    ref.set_local_codes(codes, prns)
    res_f = ref.run(xf)[0]
    assert res.tobytes() == res_f.tobytes()
    grids = _oracle_grids(xf, codes, fs, dmax, dstep, 80)
    for p in range(4):
        _check_result(res[p], grids[p], 0.01, 4, fs, dmax, dstep, 4000.0)


def test_bad_configuration_errors():
    with pytest.raises(gsdr.GsdrError) as e:
        gsdr.Acquisition(4000000, 4000, 10000, 250, pfa=2.0)
    assert e.value.code == gsdr.GSDR_E_ARG
    with pytest.raises(gsdr.GsdrError) as e:
        gsdr.Acquisition(6625000, 6625, 10000, 250)  # 6625 = 5^3 * 53: not an LDS-engine size
    assert e.value.code == gsdr.GSDR_E_UNSUPPORTED
    acq = gsdr.Acquisition(4000000, 4000, 10000, 250, max_prns=2)
    with pytest.raises(gsdr.GsdrError) as e:
        acq.run(np.zeros(4000, np.complex64))
    assert e.value.code == gsdr.GSDR_E_STATE


# Packed correlate variants (acq_pk.hip PkVariants): id -> sample rate of its
# FFT size.  Row statistic 1 (max + sum, argmax recomputed) and 2 (max only, the CFAR
# row sum by Parseval in acq_argmax_pk_kernel) must both match the oracle.
PK_VARIANTS = [(70, 4000000), (93, 16000000), (94, 16000000), (61, 8000000), (62, 2000000)]


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("variant,fs", PK_VARIANTS)
def test_packed_variants_match_oracle(monkeypatch, variant, fs, pfa):
    monkeypatch.setenv("GSDR_ACQ_CORR_VARIANT", str(variant))
    N = fs // 1000
    dmax, dstep = 10000, 250
    sats = synth.random_constellation(6, seed_offset=21 + variant)
    x = synth.gps_l1_iq(fs, N, sats, seed_offset=21 + variant)
    prns = np.array([s.prn for s in sats[:4]] + [33 - s.prn for s in sats[:2]])
    codes = _codes(prns, fs, N)
    spc = int(np.ceil(fs / 1023000.0))
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=pfa, max_prns=len(prns), num_doppler_bins=81)
    acq.set_local_codes(codes, prns)
    res = acq.run(x)[0]
    grids = _oracle_grids(x, codes, fs, dmax, dstep, 81)
    exact = sum(_check_result(res[p], grids[p], pfa, spc, fs, dmax, dstep, float(np.float32(fs) * np.float32(0.001)))
                for p in range(len(prns)))
    assert exact >= len(prns) - 1
    if pfa > 0:
        for p in range(len(prns)):
            ti, di, gmax, ip, stat = pcps.max_to_input_power_statistic(grids[p])
            if abs(stat - acq.threshold) > 1e-3 * acq.threshold:
                assert bool(res[p]["positive"]) == bool(stat > acq.threshold)

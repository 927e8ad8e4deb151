"""GPU parity of acquisition_core's non-coherent dwells (max_dwells > 1) and
bit-transition mode (pcps_acquisition.cc:615-882) against the
oracle, through the C ABI.  Per attempt and PRN the reported result is the first
dwell whose statistic crosses the threshold, else the last (:781-869)."""
import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import pcps

from acq_checks import RTOL, _check, _oracle_attempt  # noqa: F401

pytestmark = pytest.mark.gpu

FS, C = 4000000, 4000


@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_noncoherent_dwells(pfa):
    K, nat, dmax, dstep = 3, 2, 5000, 500
    sats = synth.random_constellation(6, seed_offset=11, cn0_dbhz=44.0, max_doppler=4500.0)
    x = synth.gps_l1_iq(FS, nat * K * C, sats, seed_offset=11)
    prns = np.array([s.prn for s in sats] + [31, 32])
    codes = np.stack([synth.gps_ca_sampled(int(p), FS) for p in prns])
    acq = gsdr.Acquisition(FS, C, dmax, dstep, pfa=pfa, max_prns=len(prns), max_blocks=nat, max_dwells=K)
    acq.set_local_codes(codes, prns)
    thr = pcps.threshold(pfa, C, acq.num_doppler_bins, K) if pfa > 0 else 2.5
    if pfa > 0:
        assert abs(acq.threshold - thr) <= 1e-6 * thr
    else:
        acq.set_threshold(thr)
    res = acq.run(x, nblocks=nat, stamp0=100)
    used = set()
    for a in range(nat):
        chunks = [x[(a * K + k) * C:(a * K + k + 1) * C] for k in range(K)]
        orc = _oracle_attempt(chunks, codes, pfa, acq.num_doppler_bins, dmax, dstep, False, 4, thr)
        for i in range(len(prns)):
            r = res[a, i]
            _check(r, orc[i], pfa)
            assert r["samplestamp"] == 100 + (a * K + orc[i][0]) * C
            assert r["positive"] == int(orc[i][5] > thr)
            used.add(int(r["num_dwells"]))
    assert len(used) >= 2  # some decisions before the last dwell, some at it


@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_bit_transition(pfa):
    """bit_transition_flag: consumed = 2 x 1 ms, FFT 8000 with the code in the
    second half, outputs [4000, 8000), threshold on 4000 x D cells, one dwell."""
    dmax, dstep = 5000, 250
    sats = synth.random_constellation(5, seed_offset=12, cn0_dbhz=45.0, max_doppler=4500.0)
    nb = 2
    x = synth.gps_l1_iq(FS, nb * 2 * C, sats, seed_offset=12)
    prns = np.array([s.prn for s in sats] + [30])
    codes = np.stack([np.resize(synth.gps_ca_sampled(int(p), FS), 2 * C) for p in prns])
    acq = gsdr.Acquisition(FS, 2 * C, dmax, dstep, pfa=pfa, max_prns=len(prns), max_blocks=nb, bit_transition=True,
                           max_dwells=4)
    assert acq.fft_size == 2 * C
    acq.set_local_codes(codes, prns)
    D = acq.num_doppler_bins
    thr = pcps.threshold(pfa, 2 * C, D, 4, bit_transition=True) if pfa > 0 else 2.0
    if pfa > 0:
        assert abs(acq.threshold - thr) <= 1e-6 * thr
    else:
        acq.set_threshold(thr)
    res = acq.run(x, nblocks=nb)
    for b in range(nb):
        chunk = x[b * 2 * C:(b + 1) * 2 * C]
        orc = _oracle_attempt([chunk], codes, pfa, D, dmax, dstep, True, 4, thr)
        for i in range(len(prns)):
            _check(res[b, i], orc[i], pfa)
            assert res[b, i]["samplestamp"] == b * 2 * C


@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_bit_transition_c4_four_step(monkeypatch, pfa, split):
    """Config C4's acquisition as the bench times it (pcps_acquisition.cc:85-92,
    :188-193, :671): Galileo E1 at 8 Msps, 4 ms code, bit_transition_flag -> FFT
    64000 with the code in the second half and outputs [32000, 64000), +-10 kHz /
    250 Hz (80 bins): the split register four-step (default: ROUT = 2 over a
    32000-point wave-local-row register transform, row maxima of outputs k >= N/2,
    acq_split.hip id 13) and the general (dwell) path over the packed four-step
    (GSDR_ACQ_SPLIT=0)."""
    monkeypatch.setenv("GSDR_ACQ_SPLIT", split)
    fs, C, dmax, dstep = 8000000, 32000, 10000, 250
    rng = np.random.default_rng(64)
    vis = [4, 19]
    sats = [synth.GalileoSatellite(p, float(rng.uniform(-8000, 8000)), float(rng.uniform(0, 4092)), 47.0,
                                   float(rng.uniform(0, 6.28))) for p in vis]
    x = synth.gal_e1_iq(fs, 2 * C, sats, seed_offset=64)
    prns = np.array([4, 7, 19, 30])
    codes = np.stack([np.resize(synth.gal_e1_sampled(int(p), fs), 2 * C) for p in prns])
    acq = gsdr.Acquisition(fs, 2 * C, dmax, dstep, pfa=pfa, max_prns=len(prns), bit_transition=True, sampled_ms=4,
                           ms_per_code=4, samples_per_code=float(C))
    assert acq.fft_size == 2 * C and acq.num_doppler_bins == 80
    acq.set_local_codes(codes, prns)
    D = acq.num_doppler_bins
    spc = int(np.ceil(fs / 1023000.0))
    thr = pcps.threshold(pfa, 2 * C, D, 1, bit_transition=True) if pfa > 0 else 2.0
    if pfa > 0:
        assert abs(acq.threshold - thr) <= 1e-6 * thr
    else:
        acq.set_threshold(thr)
    res = acq.run(x)
    orc = _oracle_attempt([x], codes, pfa, D, dmax, dstep, True, spc, thr, fs=fs)
    for i in range(len(prns)):
        _check(res[0, i], orc[i], pfa)
        assert res[0, i]["positive"] == int(orc[i][5] > thr)
    if pfa > 0:  # detection (not parity)
        assert {int(r["prn"]) for r in res[0] if r["positive"]} >= set(vis)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
def test_noncoherent_dwells_four_step(pfa):
    """max_dwells > 1 at a four-step size (Galileo E1, 8 Msps, 4 ms: N = 32000):
    the dwell accumulator rows of the general path on the packed four-step."""
    fs, C, K, dmax, dstep = 8000000, 32000, 2, 3000, 500
    rng = np.random.default_rng(32)
    sats = [synth.GalileoSatellite(p, float(rng.uniform(-2500, 2500)), float(rng.uniform(0, 4092)), 43.0,
                                   float(rng.uniform(0, 6.28))) for p in (4, 19)]
    x = synth.gal_e1_iq(fs, K * C, sats, seed_offset=32)
    prns = np.array([4, 7, 19])
    codes = np.stack([synth.gal_e1_sampled(int(p), fs) for p in prns])
    acq = gsdr.Acquisition(fs, C, dmax, dstep, pfa=pfa, max_prns=len(prns), max_dwells=K, sampled_ms=4,
                           ms_per_code=4, samples_per_code=float(C))
    assert acq.fft_size == C
    acq.set_local_codes(codes, prns)
    D = acq.num_doppler_bins
    spc = int(np.ceil(fs / 1023000.0))
    thr = pcps.threshold(pfa, C, D, K) if pfa > 0 else 3.0
    if pfa > 0:
        assert abs(acq.threshold - thr) <= 1e-6 * thr
    else:
        acq.set_threshold(thr)
    res = acq.run(x, stamp0=7)
    chunks = [x[k * C:(k + 1) * C] for k in range(K)]
    orc = _oracle_attempt(chunks, codes, pfa, D, dmax, dstep, False, spc, thr, fs=fs)
    for i in range(len(prns)):
        _check(res[0, i], orc[i], pfa)
        assert res[0, i]["samplestamp"] == 7 + orc[i][0] * C
        assert res[0, i]["positive"] == int(orc[i][5] > thr)


# ---------------------------------------------------------------- off the benchmark sizes
# 6 Msps: FFT 12000 with bit transition (runtime LDS plan, 1024 threads) and 6000 for the
# dwells (512 threads); 40000 = 25 x 1600 on the generic four-step (256 threads): 20 Msps
# with bit transition, 40 Msps for the dwells and the integer inputs.
OFF_GRID = (1000, 250)  # +-1000 Hz / 250 Hz: 8 Doppler rows


def _gps_case(fs, n_samples, seed, cn0):
    sats = synth.random_constellation(3, seed_offset=seed, cn0_dbhz=cn0, max_doppler=900.0)
    x = synth.gps_l1_iq(fs, n_samples, sats, seed_offset=seed)
    vis = [s.prn for s in sats]
    prns = np.array(vis + [next(p for p in range(1, 33) if p not in vis)])
    return x, prns


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("fs,variant,nthreads", [(6000000, 12, 1024), (20000000, 20, 256)])
def test_bit_transition_other_rates(fs, variant, nthreads, pfa):
    """bit_transition_flag at 6 / 20 Msps: FFT 12000 / 40000 with the code in the second
    half and outputs [N/2, N), two attempts."""
    C, (dmax, dstep), nb = fs // 1000, OFF_GRID, 2
    x, prns = _gps_case(fs, nb * 2 * C, 300 + fs // 1000000, 47.0)
    codes = np.stack([np.resize(synth.gps_ca_sampled(int(p), fs), 2 * C) for p in prns])
    acq = gsdr.Acquisition(fs, 2 * C, dmax, dstep, pfa=pfa, max_prns=len(prns), max_blocks=nb, bit_transition=True)
    plan = acq.plan
    assert acq.fft_size == 2 * C and (plan["variant"], plan["nthreads"], plan["split"]) == (variant, nthreads, 0), plan
    acq.set_local_codes(codes, prns)
    D = acq.num_doppler_bins
    spc = int(np.ceil(fs / 1023000.0))
    thr = pcps.threshold(pfa, 2 * C, D, 1, bit_transition=True) if pfa > 0 else 2.0
    if pfa > 0:
        assert abs(acq.threshold - thr) <= 1e-6 * thr
    else:
        acq.set_threshold(thr)
    res = acq.run(x, nblocks=nb)
    for b in range(nb):
        chunk = x[b * 2 * C:(b + 1) * 2 * C]
        orc = _oracle_attempt([chunk], codes, pfa, D, dmax, dstep, True, spc, thr, fs=fs)
        for i in range(len(prns)):
            _check(res[b, i], orc[i], pfa)
            assert res[b, i]["samplestamp"] == b * 2 * C
            assert res[b, i]["positive"] == int(orc[i][5] > thr)


@pytest.mark.parametrize("pfa", [0.01, 0.0])
@pytest.mark.parametrize("fs,variant,nthreads", [(6000000, 11, 512), (40000000, 20, 256)])
def test_noncoherent_dwells_other_rates(fs, variant, nthreads, pfa):
    """max_dwells = 2 at N = 6000 (runtime LDS plan) and 40000 (generic four-step): the
    accumulating general path, two attempts."""
    C, K, nat, (dmax, dstep) = fs // 1000, 2, 2, OFF_GRID
    x, prns = _gps_case(fs, nat * K * C, 310 + fs // 1000000, 46.0)
    codes = np.stack([synth.gps_ca_sampled(int(p), fs) for p in prns])
    acq = gsdr.Acquisition(fs, C, dmax, dstep, pfa=pfa, max_prns=len(prns), max_blocks=nat, max_dwells=K)
    plan = acq.plan
    assert acq.fft_size == C and (plan["variant"], plan["nthreads"], plan["split"]) == (variant, nthreads, 0), plan
    acq.set_local_codes(codes, prns)
    D = acq.num_doppler_bins
    spc = int(np.ceil(fs / 1023000.0))
    thr = pcps.threshold(pfa, C, D, K) if pfa > 0 else 3.0
    if pfa > 0:
        assert abs(acq.threshold - thr) <= 1e-6 * thr
    else:
        acq.set_threshold(thr)
    res = acq.run(x, nblocks=nat, stamp0=100)
    used = set()
    for a in range(nat):
        chunks = [x[(a * K + k) * C:(a * K + k + 1) * C] for k in range(K)]
        orc = _oracle_attempt(chunks, codes, pfa, D, dmax, dstep, False, spc, thr, fs=fs)
        for i in range(len(prns)):
            _check(res[a, i], orc[i], pfa)
            assert res[a, i]["samplestamp"] == 100 + (a * K + orc[i][0]) * C
            assert res[a, i]["positive"] == int(orc[i][5] > thr)
            used.add(int(res[a, i]["num_dwells"]))
    assert used == {1, 2}  # decisions at the first dwell and at the last


@pytest.mark.parametrize("item", [gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_integer_input_generic_four_step(item):
    """cshort / ibyte input at N = 40000 (generic four-step): the engine converts the
    interleaved integer pairs exactly, so the records are byte-identical to the
    gr_complex run of the converted samples, which is checked against the oracle."""
    fs, N, (dmax, dstep), pfa = 40000000, 40000, OFF_GRID, 0.01
    x, prns = _gps_case(fs, N, 340 + item, 50.0)
    xi = synth.to_cshort(x, 2000.0) if item == gsdr.ITEM_CSHORT else synth.to_ibyte(x, 24.0)
    xf = (xi[0::2].astype(np.float32) + 1j * xi[1::2].astype(np.float32)).astype(np.complex64)
    codes = np.stack([synth.gps_ca_sampled(int(p), fs) for p in prns])
    acq = gsdr.Acquisition(fs, N, dmax, dstep, pfa=pfa, max_prns=len(prns), item_type=item)
    assert acq.plan["variant"] == 20
    acq.set_local_codes(codes, prns)
    res = acq.run(xi)[0]
    ref = gsdr.Acquisition(fs, N, dmax, dstep, pfa=pfa, max_prns=len(prns))
    ref.set_local_codes(codes, prns)
    res_f = ref.run(xf)[0]
    assert res.tobytes() == res_f.tobytes()
    orc = _oracle_attempt([xf], codes, pfa, acq.num_doppler_bins, dmax, dstep, False, int(np.ceil(fs / 1023000.0)),
                          acq.threshold, fs=fs)
    for i in range(len(prns)):
        _check(res[i], orc[i], pfa)
        assert res[i]["positive"] == int(orc[i][5] > acq.threshold)

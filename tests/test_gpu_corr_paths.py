"""The multicorrelator paths test_gpu_corr.py does not reach (corr.hip).

Exact integer probe (tests/corr_checks.py): zero carrier, integer IQ and replica, so
the taps must equal int64 sums bit for bit.  It pins the index the correlate kernel
computes itself (raw_index, the chunk's LDS span and its wrap, the global fallback
for spans over the cap and for step <= 0, the high-dynamics index across a chunk
boundary), both float associations on parameters where they differ, the cshort and
ibyte entry of gsdr_corr_run, and the batch machinery: jobs of mixed length in one
grid, windows that leave the IQ buffer, the cross-chunk counters re-armed launch
after launch, the workspace growing past 64 jobs, device job tables and their guard.
Every batch output is pre-filled with NaN.

Tolerance tests against the oracle's fp64 companions, vnorm_rel <= 1e-5 (the bound
test_gpu_corr.py holds the real-code path to; the complex and high-dynamics paths
share its fp64-anchored phase and fp32 accumulation): complex codes, high dynamics,
the generic association with a carrier, a 2.5 rad/sample carrier step, and device
job tables (2e-5, the device-side rotator model's bound in
test_run_epochs_matches_per_epoch_batches).
"""
import numpy as np
import pytest

import gsdr
from gsdr import synth
from oracle import volk

import corr_checks as cc
from conftest import vnorm_rel

pytestmark = pytest.mark.gpu

ASSOCS = [cc.GENERIC, cc.AVX]
B1I_STEP = cc.f32(2.046e6 / 2e6)  # BeiDou B1I at 2 Msps: the replica outruns the samples


def _one(ch, N, rem, step, assoc=cc.AVX, rate=0.0, seed=1):
    """One job of N samples through run_batch against the probe's sums."""
    iq = cc.probe_iq(N, seed)
    corr = cc.correlator([ch], N, ch.K, assoc)
    jobs = cc.job_table([cc.job(0, N, 0, rem, step, rate)])
    got = cc.launch(corr, jobs, cc.to_device(cc.iq_items(iq)), N)
    cc.assert_rows_exact(got, cc.expected_rows(iq, [ch], jobs, assoc))


# --- A. exact probe: the index and the span ---------------------------------------


@pytest.mark.parametrize("assoc", ASSOCS)
@pytest.mark.parametrize("N", [4000, 8197])
def test_probe_lds_span_both_associations(N, assoc):
    """lds_single (one chunk) and lds_multi_wrap (2 full chunks + 5; every span is
    longer than the code, so the staging wraps it) through gsdr_corr_run."""
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS)
    iq = cc.probe_iq(N, 1)
    want = cc.expected_both_assocs(iq, ch, cc.AG_REM, cc.AG_STEP, N)
    assert max(cc.chunk_spans(ch, cc.AG_REM, cc.AG_STEP, N, assoc)) <= cc.SPAN_CAP
    corr = cc.correlator([ch], N, ch.K, assoc)
    got = corr.run(0, cc.iq_items(iq), 0.0, 0.0, cc.AG_REM, cc.AG_STEP, N)
    np.testing.assert_array_equal(got, want[assoc])


@pytest.mark.parametrize("item_type", [gsdr.ITEM_CSHORT, gsdr.ITEM_IBYTE])
def test_probe_run_item_types(item_type):
    """gsdr_corr_run with cshort and ibyte items: the integer IQ is the native input."""
    N = 8197
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS)
    iq = cc.probe_iq(N, 1)
    want = cc.expected_both_assocs(iq, ch, cc.AG_REM, cc.AG_STEP, N)
    for assoc in ASSOCS:
        corr = cc.correlator([ch], N, ch.K, assoc)
        got = corr.run(0, cc.iq_items(iq, item_type), 0.0, 0.0, cc.AG_REM, cc.AG_STEP, N, item_type=item_type)
        np.testing.assert_array_equal(got, want[assoc])


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("shifts,span", [([0.0], cc.SPAN_CAP), ([0.0, 1.0], cc.SPAN_CAP + 1)])
def test_probe_span_cap(shifts, span, cplx):
    """cap_exact: a span of 4096 entries is staged in LDS (a complex replica fills the
    buffer to its last float).  cap_plus_one: 4097 is the first span read from global."""
    ch = cc.Chan(cc.probe_code(1023, 3, cplx), shifts)
    assert cc.chunk_spans(ch, 0.0, 1.0, 4096) == [span]
    _one(ch, 4096, 0.0, 1.0)


@pytest.mark.parametrize("cplx", [False, True])
def test_probe_global_and_lds_chunks_in_one_job(cplx):
    """global_mixed: chunk 0 spans 4191 entries (global), chunk 1 spans 103 (LDS)."""
    ch = cc.Chan(cc.probe_code(2046, 4, cplx), [-0.5, 0.0, 0.5])
    assert cc.chunk_spans(ch, 0.0, B1I_STEP, 4196) == [4191, 103]
    _one(ch, 4196, 0.0, B1I_STEP)


@pytest.mark.parametrize("step", [0.0, -cc.AG_STEP])
def test_probe_step_not_positive(step):
    """step_zero, step_negative: no monotone span, the global fallback; the negative
    step walks the raw index down to about -1050."""
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS)
    if step < 0:
        assert cc.raw_indices(ch, cc.AG_REM, step, [4099]).min() < -ch.L
    for assoc in ASSOCS:
        _one(ch, 4100, cc.AG_REM, step, assoc)


def test_probe_high_dynamics_across_chunks():
    """hd_multi: the rate term is active (it moves 2855 of the 21980 indices) and taps
    1..4 are tap 0 shifted by 2, 3, 3 and 5 samples modulo N, across the chunk boundary."""
    N, rate = 4396, 2e-8
    ch = cc.Chan(cc.probe_code(cc.AG_L, 1), cc.AG_SHIFTS, high_dyn=True)
    moved = cc.indices(ch, cc.AG_REM, cc.AG_STEP, N, rate=rate) != cc.indices(ch, cc.AG_REM, cc.AG_STEP, N)
    assert moved.sum() > 2000
    _one(ch, N, cc.AG_REM, cc.AG_STEP, rate=rate)


# --- A. exact probe: batches --------------------------------------------------------

IQ_ITEMS = 20000
MIXED_LENGTHS = [0, 1, 4095, 4096, 4097, 8192, 12288]


def _two_channels():
    return [cc.Chan(cc.probe_code(cc.AG_L, 5), [0.1]), cc.Chan(cc.probe_code(cc.AG_L, 6), cc.AG_SHIFTS)]


def _mixed_jobs():
    """Every length on both channels, interleaved, each with its own window and code phase."""
    rng = np.random.default_rng(77)
    rows = []
    for n in MIXED_LENGTHS:
        for c in (0, 1):
            rows.append(cc.job(c, n, int(rng.integers(0, IQ_ITEMS - n)), cc.f32(rng.uniform(-0.5, 0.5)),
                               cc.f32(cc.AG_STEP * (1 + rng.uniform(-1e-4, 1e-4)))))
    return cc.job_table(rows)


def test_probe_mixed_lengths_and_rearm():
    """Jobs of 0 to 3 chunks in one grid of 3 chunk columns, three launches in a row on
    one handle (the counters of launch 1 must be re-armed for 2 and 3), then the same
    through run_epochs with 3 epochs of multi-chunk jobs."""
    chans = _two_channels()
    iq = cc.probe_iq(IQ_ITEMS, 7)
    dev = cc.to_device(cc.iq_items(iq))
    corr = cc.correlator(chans, 3 * cc.CHUNK, 8)
    jobs = _mixed_jobs()
    want = cc.expected_rows(iq, chans, jobs)
    for j, w in zip(jobs, want):
        if j["n_samples"] == 0:
            assert not w.any()
    for launch in range(3):
        cc.assert_rows_exact(cc.launch(corr, jobs, dev, IQ_ITEMS), want)
    # epochs: 3 x 4 jobs, each of 2 or 3 chunks, the job slots' counters used 3 times
    rng = np.random.default_rng(78)
    rows = [cc.job(int(rng.integers(0, 2)), int(rng.integers(cc.CHUNK + 1, 3 * cc.CHUNK + 1)),
                   int(rng.integers(0, 7000)), cc.f32(rng.uniform(-0.5, 0.5))) for _ in range(12)]
    ejobs = cc.job_table(rows)
    got = cc.launch(corr, ejobs, dev, IQ_ITEMS, how="epochs", epochs=3)
    cc.assert_rows_exact(got, cc.expected_rows(iq, chans, ejobs))
    # and the host path again after the device tables
    cc.assert_rows_exact(cc.launch(corr, jobs, dev, IQ_ITEMS), want)


def test_probe_windows_outside_the_buffer():
    """Samples outside [0, iq_items) read as zeros: a window that starts before the
    buffer, ones that run off its end, and ones wholly outside it."""
    chans = _two_channels()
    n_items = 9000
    iq = cc.probe_iq(n_items, 8)
    rows = [cc.job(1, 300, -100, 0.2), cc.job(1, 5000, -100, -0.3), cc.job(0, 4097, -4096, 0.1),
            cc.job(1, 200, n_items - 50, 0.4), cc.job(1, 8192, n_items - 50, 0.0), cc.job(0, 8192, n_items - 4097, 0.3),
            cc.job(1, 100, n_items, 0.1), cc.job(1, 5000, n_items + 12345, 0.1), cc.job(0, 700, -700, 0.1),
            cc.job(1, 600, -5000, 0.1)]
    jobs = cc.job_table(rows)
    want = cc.expected_rows(iq, chans, jobs)
    assert all(not w.any() for w in want[6:]) and all(w.any() for w in want[:6])
    corr = cc.correlator(chans, 2 * cc.CHUNK, 5)
    for item_type in (gsdr.ITEM_GR_COMPLEX, gsdr.ITEM_IBYTE):
        dev = cc.to_device(cc.iq_items(iq, item_type))
        cc.assert_rows_exact(cc.launch(corr, jobs, dev, n_items, item_type=item_type), want)


def test_probe_workspace_growth():
    """10 jobs, 130 jobs (the job, partial and counter workspace is reallocated past
    64), 10 jobs again, on one handle; mostly short jobs, a few multi-chunk."""
    chans = _two_channels()
    iq = cc.probe_iq(IQ_ITEMS, 9)
    dev = cc.to_device(cc.iq_items(iq))
    corr = cc.correlator(chans, 2 * cc.CHUNK + 5, 5)
    rng = np.random.default_rng(79)
    for njobs in (10, 130, 10):
        rows = []
        for j in range(njobs):
            n = int(rng.integers(cc.CHUNK + 1, 2 * cc.CHUNK + 6)) if j % 9 == 4 else int(rng.integers(0, 257))
            rows.append(cc.job(int(rng.integers(0, 2)), n, int(rng.integers(0, IQ_ITEMS - n)),
                               cc.f32(rng.uniform(-0.5, 0.5))))
        jobs = cc.job_table(rows)
        cc.assert_rows_exact(cc.launch(corr, jobs, dev, IQ_ITEMS), cc.expected_rows(iq, chans, jobs))


def test_probe_device_table_equals_host_table():
    chans = _two_channels()
    iq = cc.probe_iq(IQ_ITEMS, 7)
    dev = cc.to_device(cc.iq_items(iq, gsdr.ITEM_CSHORT))
    corr = cc.correlator(chans, 3 * cc.CHUNK, 8)
    jobs = _mixed_jobs()
    host = cc.launch(corr, jobs, dev, IQ_ITEMS, item_type=gsdr.ITEM_CSHORT)
    device = cc.launch(corr, jobs, dev, IQ_ITEMS, how="device", item_type=gsdr.ITEM_CSHORT)
    cc.assert_rows_exact(device, cc.expected_rows(iq, chans, jobs))
    np.testing.assert_array_equal(device.view(np.uint32), host.view(np.uint32))


def test_probe_device_table_guard():
    """The inputs the kernel's guard names: a channel outside [0, nchan) or a length
    that is negative or needs more chunks than the grid holds gives a NaN row of
    max_taps entries and leaves the job slot's counter alone; its neighbours are exact."""
    chans = _two_channels()
    iq = cc.probe_iq(IQ_ITEMS, 10)
    dev = cc.to_device(cc.iq_items(iq))
    corr = cc.correlator(chans, cc.CHUNK, 5)
    bad = {1: cc.job(-1, 4096, 10, 0.1), 3: cc.job(2, 100, 20, 0.1), 4: cc.job(1, -1, 30, 0.1),
           6: cc.job(0, 4097, 40, 0.1)}
    good = {0: cc.job(1, 4096, 0, 0.2), 2: cc.job(0, 4000, 100, -0.2), 5: cc.job(1, 1, 5, 0.3),
            7: cc.job(1, 2500, 17000, 0.0), 8: cc.job(0, 0, 0, 0.0)}
    jobs = cc.job_table([{**bad, **good}[j] for j in range(9)])
    for rep in range(2):
        got = cc.launch(corr, jobs, dev, IQ_ITEMS, how="device")
        for j in bad:
            assert np.isnan(got[j].real).all() and np.isnan(got[j].imag).all(), (j, got[j])
        ok = sorted(good)
        cc.assert_rows_exact(got[ok], cc.expected_rows(iq, chans, jobs[ok]))
    # an all-valid multi-chunk batch on another handle afterwards
    corr2 = cc.correlator(chans, 2 * cc.CHUNK, 5)
    jobs2 = cc.job_table([cc.job(j % 2, 8192 - 3 * j, 50 * j, 0.05 * j) for j in range(9)])
    for rep in range(2):
        got = cc.launch(corr2, jobs2, dev, IQ_ITEMS, how="device")
        cc.assert_rows_exact(got, cc.expected_rows(iq, chans, jobs2))


# --- B. tolerance against the fp64 companions ---------------------------------------


def _report(name, got, exact, ref=None, bound=1e-5):
    g = vnorm_rel(got, exact)
    line = "%s: GPU vs exact %.2e (bound %.0e)" % (name, g, bound)
    if ref is not None:
        line += ", reference vs exact %.2e (bound 1e-04)" % vnorm_rel(ref, exact)
    print(line)
    return g


@pytest.mark.parametrize("item_type", [gsdr.ITEM_GR_COMPLEX, gsdr.ITEM_CSHORT])
@pytest.mark.parametrize("doppler", [800.0, -800.0])
def test_complex_codes_vs_exact(doppler, item_type):
    fs, N = 4e6, 8197
    code = cc.complex_code(9)
    x = cc.strong_signal(fs, N, 9, doppler, seed=3)
    host = x
    if item_type == gsdr.ITEM_CSHORT:
        host = synth.to_cshort(x, 1000.0)
        x = (host[0::2].astype(np.float32) + 1j * host[1::2].astype(np.float32)).astype(np.complex64)
    args = (0.7, cc.f32(2 * np.pi * doppler / fs), 0.05, cc.f32(1.023e6 / fs))
    corr = gsdr.Correlator(1, N, max_taps=5)
    corr.set_local_code_and_taps(0, code, cc.SHIFTS5)
    got = corr.run(0, host, *args, N, item_type=item_type)
    exact = volk.multicorrelator_complex_codes_exact(x, code, cc.SHIFTS5, *args, N)
    ref = volk.multicorrelator_complex_codes(x, code, cc.SHIFTS5, *args, N)
    assert _report("complex codes %+.0f Hz item %d" % (doppler, item_type), got, exact, ref) <= 1e-5


@pytest.mark.parametrize("N", [4000, 4396])
def test_high_dynamics_vs_exact(N):
    fs = 4e6
    code = synth.gps_ca_chips(11)
    x = cc.strong_signal(fs, N, 11, 2100.0, seed=4)
    kw = dict(carr_rate=2e-9, code_rate=1e-10)
    args = (0.1, cc.f32(2 * np.pi * 2100.0 / fs), 0.05, cc.f32(1.023e6 / fs))
    corr = gsdr.Correlator(1, N, max_taps=5)
    corr.set_local_code_and_taps(0, code, cc.SHIFTS5)
    corr.set_high_dynamics_resampler(0, True)
    got = corr.run(0, x, *args, N, **kw)
    exact = volk.multicorrelator_real_codes_hd_exact(x, code, cc.SHIFTS5, *args, N, **kw)
    ref = volk.multicorrelator_real_codes(x, code, cc.SHIFTS5, *args, N, high_dyn=True, **kw)
    assert _report("high dynamics N=%d" % N, got, exact, ref) <= 1e-5


def test_generic_association_with_carrier_vs_exact():
    fs, N = 4e6, 8197
    code = synth.gps_ca_chips(5)
    x = cc.strong_signal(fs, N, 5, 1523.25, seed=5)
    args = (-1.3, cc.f32(2 * np.pi * 1523.25 / fs), cc.AG_REM, cc.AG_STEP)
    corr = gsdr.Correlator(1, N, max_taps=5)
    corr.set_resampler_assoc(cc.GENERIC)
    corr.set_local_code_and_taps(0, code, cc.AG_SHIFTS)
    got = corr.run(0, x, *args, N)
    exact = volk.multicorrelator_real_codes_exact(x, code, cc.AG_SHIFTS, *args, N, assoc=cc.GENERIC)
    ref = volk.multicorrelator_real_codes(x, code, cc.AG_SHIFTS, *args, N, assoc=cc.GENERIC)
    assert _report("generic association", got, exact, ref) <= 1e-5


def test_large_carrier_step_vs_exact():
    """An IF configuration, 2.5 rad per sample.  Against the exact value only: the
    reference's fp32 phasor recursion is the less precise one at this step (5.1e-6
    from the exact value on this input)."""
    fs, N = 4e6, 8197
    f_if = 2.5 * fs / (2 * np.pi)
    code = synth.gps_ca_chips(5)
    x = cc.strong_signal(fs, N, 5, f_if, seed=6)
    args = (0.4, cc.f32(2 * np.pi * f_if / fs), 0.05, cc.f32(1.023e6 / fs))
    assert abs(args[1] - 2.5) < 1e-6
    corr = gsdr.Correlator(1, N, max_taps=5)
    corr.set_local_code_and_taps(0, code, cc.SHIFTS5)
    got = corr.run(0, x, *args, N)
    exact = volk.multicorrelator_real_codes_exact(x, code, cc.SHIFTS5, *args, N)
    assert abs(exact[2]) > 0.2 * N  # the carrier is wiped off: the prompt tap is 20 x a noise-only sum
    assert _report("carrier step 2.5 rad", got, exact) <= 1e-5


def test_device_table_with_carrier_multichunk_cshort():
    """run_batch_device derives the rotator angles on the device (no host model)."""
    fs, total = 4e6, 20000
    sats = [synth.Satellite(5, 1523.25, 0.0, 55.0), synth.Satellite(9, -2210.5, 0.0, 55.0)]
    host = synth.to_cshort(synth.gps_l1_iq(fs, total, sats, seed_offset=8), 1000.0)
    xf = (host[0::2].astype(np.float32) + 1j * host[1::2].astype(np.float32)).astype(np.complex64)
    chans = [cc.Chan(synth.gps_ca_chips(s.prn), cc.SHIFTS5) for s in sats]
    corr = cc.correlator(chans, 3 * cc.CHUNK, 5)
    step = cc.f32(1.023e6 / fs)
    jobs = np.zeros(4, gsdr.CORR_JOB_DTYPE)
    for j, (c, n, k) in enumerate([(0, 8197, 0), (1, 12288, 1), (0, 4097, 2), (1, 5000, 3)]):
        # windows starting k code periods in: the prompt tap stays aligned
        jobs[j] = (c, n, 4000 * k, 0.3 * j - 0.5, np.float32(2 * np.pi * sats[c].doppler_hz / fs), 0.0, 0.02 * j, step,
                   0.0)
    got = cc.launch(corr, jobs, cc.to_device(host), total, how="device", item_type=gsdr.ITEM_CSHORT)
    for j, job in enumerate(jobs):
        n, off = int(job["n_samples"]), int(job["sample_offset"])
        exact = volk.multicorrelator_real_codes_exact(
            xf[off:off + n], chans[job["channel"]].code, cc.SHIFTS5, float(job["rem_carr_phase_rad"]),
            float(job["carr_phase_step_rad"]), float(job["rem_code_phase_chips"]), step, n)
        assert abs(exact[2]) > 100.0 * n  # strong signal (cshort scale 1000)
        assert _report("device table job %d" % j, got[j, :5], exact, bound=2e-5) <= 2e-5

"""The host mirror of pcps_acquisition_fine_doppler_cc (host/pcps_acquisition_fine_doppler_mi355x.cc
and its adapter), built by the block factory from a .conf and driven through its state machine
by host/tests/fine_doppler_selftest.cc with 1 ms items and max_dwells = 2.

The program reports the state before every work() call, what each call consumed, the event and
the Gnss_Synchro acquisition fields; they are compared with a restatement of the whole block:
the coarse grid accumulated over the two dwell blocks by oracle.pcps (first / second peak, the
block's floor(2 doppler_max / doppler_step) rows), then tests/fine_checks.py on the 10 ms that
start at the first dwell block."""
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest

from gsdr import synth
from oracle import pcps

import fine_checks as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "fine_doppler_selftest")
FS, N, DMAX, DSTEP, DWELLS = 4000000, 4000, 5000, 500, 2
PRESENT, ABSENT = 7, 31
THRESHOLD = 2.5
MAT_NAMES = {"acq_grid", "doppler_max", "doppler_step", "d_positive_acq", "acq_doppler_hz", "acq_delay_samples",
             "test_statistic", "threshold", "input_power", "sample_counter", "PRN"}


@functools.lru_cache(maxsize=None)
def stream():
    """28 ms with two satellites whose Dopplers are whole fine bins near a coarse row (1012.5 and
    -2487.5 Hz) and no navigation bit edge."""
    sats = [synth.Satellite(PRESENT, 81 * 12.5, 1233 * 1023.0 / N, 47.0, phase=0.7, bit_period_ms=1000),
            synth.Satellite(17, -199 * 12.5, 2500 * 1023.0 / N, 46.0, phase=2.1, bit_period_ms=1000)]
    return synth.gps_l1_iq(FS, 28 * N, sats, seed_offset=41)


@functools.lru_cache(maxsize=None)
def block_restatement(prn, start):
    """The attempt that begins with the state-0 call at item `start`."""
    x = stream()
    code = synth.gps_ca_sampled(prn, FS)
    D = abs(2 * DMAX) // DSTEP  # :134
    wipe = pcps.doppler_wipeoffs(FS, N, DMAX, DSTEP, D)
    cf = pcps.fft_code(code, N, N)
    first = start + N
    M = np.zeros((D, N), np.float32)
    for k in range(DWELLS):
        M = M + pcps.magnitude_grid(x[first + k * N:first + (k + 1) * N], wipe, cf).astype(np.float32)
    spc = int(math.ceil(9.7752e-07 * float(np.float32(FS))))  # :242
    ti, di, p1, p2, stat = pcps.first_vs_second_peak_statistic(M.copy(), spc, N)
    top = np.partition(M.ravel(), M.size - 2)[M.size - 2:]
    r = {"grid": M, "ti": int(ti), "doppler": DSTEP * int(di) - DMAX, "stat": float(stat),
         "stamp": first + DWELLS * N, "coarse_margin": float((top[1] - top[0]) / top[1]),
         "positive": float(stat) > THRESHOLD}
    if r["positive"]:
        r["fine"] = fc.estimate_doppler(x[first:first + 10 * N], code, r["ti"], float(r["doppler"]), FS)
    return r


def run_selftest(tmp_path, prn, attempts, ring=0, dump=False, implementation="GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_MI355X"):
    iq = tmp_path / "iq.dat"
    stream().tofile(iq)
    conf = tmp_path / "fine.conf"
    conf.write_text("\n".join([
        "; fine-Doppler acquisition on the MI355X engine",
        "[GNSS-SDR]",
        "GNSS-SDR.internal_fs_sps=%d" % FS,
        "Acquisition_1C.implementation=%s" % implementation,
        "Acquisition_1C.item_type=gr_complex",
        "Acquisition_1C.doppler_max=%d" % DMAX,
        "Acquisition_1C.doppler_step=%d" % DSTEP,
        "Acquisition_1C.max_dwells=%d ; two 1 ms blocks" % DWELLS,
        "Acquisition_1C.dump=%s" % ("true" if dump else "false"),
        "Acquisition_1C.dump_filename=%s" % (tmp_path / "fine_acq.mat"),
    ]) + "\n")
    r = subprocess.run([EXE, str(conf), str(iq), str(prn), repr(THRESHOLD), str(attempts), str(ring)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def check_attempt(a, ref, start):
    assert a["start"] == start
    assert ref["coarse_margin"] >= fc.MIN_MARGIN
    if ref["positive"]:
        # state 0, two dwells, the decision, eight 1 ms items up to 10 ms, the event
        assert a["states"] == [0, 1, 1, 2] + [3] * 8 + [4]
        assert a["consumed"] == [N, N, N, 0] + [N] * 8 + [N]
        assert a["event"] == 1
        f = ref["fine"]
        assert f["margin"] >= fc.MIN_MARGIN
        assert a["fine_index"] == f["index"] and a["fine_accepted"] == f["accepted"] == 1
        assert a["acq_doppler_hz"] == f["doppler_hz"]
        assert abs(f["doppler_hz"] - ref["doppler"]) < 1000 and f["doppler_hz"] != ref["doppler"]
    else:
        assert a["states"] == [0, 1, 1, 2, 5]
        assert a["consumed"] == [N, N, N, 0, N]
        assert a["event"] == 2
        assert a["acq_doppler_hz"] == float(ref["doppler"])
    assert a["end_state"] == 0
    assert a["sample_counter"] == start + sum(a["consumed"])
    assert a["acq_delay_samples"] == float(ref["ti"])  # the raw row index
    assert a["acq_samplestamp_samples"] == ref["stamp"]
    assert a["acq_doppler_step"] == DSTEP
    assert abs(a["test_statistic"] - ref["stat"]) <= fc.RTOL * ref["stat"]
    assert a["mag"] == int(a["test_statistic"])


def test_positive_acquisition_with_dump(tmp_path):
    rc, out = run_selftest(tmp_path, PRESENT, 1, dump=True)
    assert rc == 0 and out["built"] and out["implementation"] == "GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_MI355X"
    assert (out["item_size"], out["fft_size"], out["num_doppler_points"], out["max_dwells"], out["doppler_max"]) == \
        (8, N, 20, DWELLS, DMAX)
    ref = block_restatement(PRESENT, 0)
    assert ref["positive"] and ref["ti"] == 1234 and ref["doppler"] == 1000
    assert ref["fine"]["doppler_hz"] == 1012.5
    a = out["attempts"][0]
    check_attempt(a, ref, 0)
    # the .mat dump: the reference's variable names, written at the event
    assert a["dump"].endswith("fine_acq_G_1C_ch_0_1_sat_%d.mat" % PRESENT) and os.path.exists(a["dump"])
    sio = pytest.importorskip("scipy.io")
    m = sio.loadmat(a["dump"])
    assert {k for k in m if not k.startswith("__")} == MAT_NAMES
    assert m["acq_grid"].shape == (N, 20) and m["acq_grid"].dtype == np.float32
    assert np.max(np.abs(m["acq_grid"].T.astype(np.float64) - ref["grid"])) <= fc.RTOL * float(ref["grid"].max())
    assert int(m["d_positive_acq"][0, 0]) == 1 and int(m["PRN"][0, 0]) == PRESENT
    assert float(m["acq_doppler_hz"][0, 0]) == 1012.5 and float(m["acq_delay_samples"][0, 0]) == 1234.0
    assert float(m["input_power"][0, 0]) == 0.0 and float(m["threshold"][0, 0]) == THRESHOLD
    assert int(m["doppler_max"][0, 0]) == DMAX and int(m["doppler_step"][0, 0]) == DSTEP
    assert int(m["sample_counter"][0, 0]) == 11 * N  # at the state-4 call, before it consumes its item


def test_negative_acquisition(tmp_path):
    rc, out = run_selftest(tmp_path, ABSENT, 1)
    assert rc == 0
    ref = block_restatement(ABSENT, 0)
    assert not ref["positive"]
    check_attempt(out["attempts"][0], ref, 0)


def test_accepted_then_reset_second_attempt(tmp_path):
    """reset() after the positive event: the second attempt runs on the samples that follow,
    its grid, buffer and counters started afresh."""
    rc, out = run_selftest(tmp_path, PRESENT, 2)
    assert rc == 0 and len(out["attempts"]) == 2
    check_attempt(out["attempts"][0], block_restatement(PRESENT, 0), 0)
    ref = block_restatement(PRESENT, 12 * N)
    assert ref["positive"]
    check_attempt(out["attempts"][1], ref, 12 * N)
    assert out["attempts"][1]["acq_samplestamp_samples"] == 15 * N


def test_ring_path_equals_buffer_path(tmp_path):
    """With a device ring attached the block hands the window's first sample to the stream form
    instead of copying: the same records."""
    rc, host = run_selftest(tmp_path, PRESENT, 2)
    rc2, ring = run_selftest(tmp_path, PRESENT, 2, ring=1)
    assert rc == 0 and rc2 == 0
    assert ring["attempts"] == host["attempts"]


def test_factory_does_not_answer_unknown_key(tmp_path):
    rc, out = run_selftest(tmp_path, PRESENT, 1, implementation="GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_Nowhere")
    assert rc == 1 and out == {"built": False}

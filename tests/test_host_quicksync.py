"""The host mirror of pcps_quicksync_acquisition_cc (host/pcps_quicksync_acquisition_mi355x.cc and
its adapter host/gps_l1_ca_pcps_quicksync_acquisition_mi355x.cc), built by the block factory from
a .conf and driven through its state machine by host/tests/quicksync_acquisition_selftest.cc, from
a host buffer and from the device ring.

Shape: 4 Msps, 4000 samples per code, folding factor 4 (the reference's default at this rate, with
coherent_integration_time_ms = 4): a 1000-point grid over items of 16000 samples, +-1000 Hz /
250 Hz.  The program reports, for every work() call, the state before it, what it consumed, the
event and the Gnss_Synchro acquisition fields; they are compared call by call with the restatement
of the whole block in tests/quicksync_checks.py (RefBlock).
  STRONG  in every item: positive at the first dwell; with bit_transition_flag decided only after
          the second dwell, on that dwell's statistic;
  ABSENT  negative after max_dwells = 2.
The threshold is chosen on the CPU from the restatement's statistics of every item: the geometric
mean of ABSENT's largest and STRONG's smallest, which must lie a factor 2 from both."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from gsdr import synth

import quicksync_checks as qc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "quicksync_acquisition_selftest")
FS, SPC, P, DMAX, DSTEP, DWELLS, ITEMS = 4000000, 4000, 4, 1000, 250, 2, 12
NF, L = SPC // P, P * SPC
STRONG, ABSENT = 11, 30
KEY = "GPS_L1_CA_PCPS_QuickSync_Acquisition_MI355X"


@functools.lru_cache(maxsize=None)
def code(prn):
    return synth.gps_ca_sampled(prn, FS).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def stream():
    """ITEMS items with STRONG in each (row 6 = 500 Hz, delay 2921: candidate 2, folded phase 921)."""
    rows = qc.doppler_rows(DMAX, DSTEP)
    rng = np.random.default_rng(synth.SEED + 7500)
    n = np.arange(ITEMS * L)
    c = code(STRONG).astype(np.complex128)[(n - 2921) % SPC]
    x = np.sqrt(200.0 * P / SPC) * c * np.exp(1j * (2 * np.pi * rows[6] * n / FS + 0.3))
    x = x + (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n))) * np.sqrt(0.5)
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def item_records(prn):
    x = stream()
    return [qc.item_record(x[i * L:(i + 1) * L], FS, DMAX, DSTEP, code(prn), P, i * L) for i in range(ITEMS)]


@functools.lru_cache(maxsize=None)
def threshold():
    strong = min(r["rec"]["test_statistic"] for r in item_records(STRONG))
    absent = max(r["rec"]["test_statistic"] for r in item_records(ABSENT))
    thr = float(np.float32(np.sqrt(strong * absent)))
    assert absent * 2.0 <= thr <= strong / 2.0, (absent, thr, strong)
    return thr


@functools.lru_cache(maxsize=None)
def restatement(prn, attempts, per_call=1, bit_transition=False):
    blk = qc.RefBlock(FS, SPC, P, DMAX, DSTEP, DWELLS, threshold(), bit_transition, code(prn))
    return qc.run_attempts(blk, stream(), attempts, per_call)


def run_selftest(tmp_path, prn, attempts, ring=0, per_call=1, extra=(), ms=4, thr=None, step=DSTEP):
    iq = tmp_path / "iq.dat"
    stream().tofile(iq)
    conf = tmp_path / "quicksync.conf"
    conf.write_text("\n".join([
        "; QuickSync GPS L1 C/A acquisition on the MI355X engine",
        "[GNSS-SDR]",
        "GNSS-SDR.internal_fs_sps=%d" % FS,
        "Acquisition_1C.implementation=%s" % KEY,
        "Acquisition_1C.item_type=gr_complex",
        "Acquisition_1C.coherent_integration_time_ms=%d" % ms,
        "Acquisition_1C.doppler_max=%d" % DMAX,
        "Acquisition_1C.doppler_step=%d" % step,
        "Acquisition_1C.max_dwells=%d" % DWELLS,
    ] + list(extra)) + "\n")
    thr = threshold() if thr is None else thr
    r = subprocess.run([EXE, str(conf), str(iq), str(prn), repr(thr), str(attempts), str(ring), str(per_call)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def check(out, ref, bit_transition=False):
    assert out["built"] and out["implementation"] == KEY
    assert (out["item_samples"], out["fft_size"], out["folding_factor"], out["num_doppler_bins"], out["max_dwells"],
            out["doppler_max"], out["sampled_ms"], out["bit_transition_flag"]) == \
        (L, NF, P, 9, DWELLS, DMAX, P, int(bit_transition))
    assert len(out["attempts"]) == len(ref)
    for a, w in zip(out["attempts"], ref):
        assert [c["state"] for c in a["calls"]] == [c["state"] for c in w["calls"]]
        assert [c["consumed"] for c in a["calls"]] == [c["consumed"] for c in w["calls"]]
        assert [c["event"] for c in a["calls"]] == [c["event"] for c in w["calls"]]
        assert (a["event"], a["end_state"], a["sample_counter"]) == (w["event"], w["end_state"], w["sample_counter"])
        for c, r in zip(a["calls"], w["calls"]):
            assert c["acq_delay_samples"] == r["acq_delay_samples"], (c, r)
            assert c["acq_doppler_hz"] == r["acq_doppler_hz"], (c, r)
            assert c["acq_samplestamp_samples"] == r["acq_samplestamp_samples"], (c, r)  # the end of the item
            assert c["acq_doppler_step"] == r["acq_doppler_step"], (c, r)
            for k in ("mag", "input_power", "test_statistic"):
                assert abs(c[k] - r[k]) <= qc.RTOL * abs(r[k]), (k, c, r)


def _pin_margins(prn):
    for rec in item_records(prn):
        assert min(rec["margins"].values()) >= qc.MIN_MARGIN, rec["margins"]


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("prn", [STRONG, ABSENT])
def test_block_against_restatement(tmp_path, prn, ring):
    """Two attempts, two items offered per call."""
    attempts, per_call = 2, 2
    ref = restatement(prn, attempts, per_call)
    _pin_margins(prn)
    events = [a["event"] for a in ref]
    dwells = [sum(c["state"] == 1 for c in a["calls"]) for a in ref]
    if prn == STRONG:
        assert events == [1, 1] and dwells == [1, 1]
        work = ref[0]["calls"][1]
        # state 0 took two items; the third is the dwell, stamped at its end
        assert (work["acq_delay_samples"], work["acq_doppler_hz"], work["acq_samplestamp_samples"]) == (2921.0, 500.0, 3 * L)
    else:
        assert events == [2, 2] and dwells == [2, 2]
    rc, out = run_selftest(tmp_path, prn, attempts, ring, per_call)
    assert rc == 0
    check(out, ref)


@pytest.mark.parametrize("ring", [0, 1])
def test_bit_transition_decides_after_the_second_dwell(tmp_path, ring):
    """bit_transition_flag forces max_dwells = 2 (the .conf asks for 1): STRONG, above the threshold
    in dwell 0 already, is published only by the call after dwell 1, with dwell 1's fields."""
    ref = restatement(STRONG, 2, 2, True)
    _pin_margins(STRONG)
    assert [a["event"] for a in ref] == [1, 1]
    assert [[c["state"] for c in a["calls"]] for a in ref] == [[0, 1, 1, 2], [0, 1, 1, 2]]
    first = ref[0]["calls"]
    assert first[1]["test_statistic"] > threshold() and first[1]["event"] == 0
    assert first[2]["acq_samplestamp_samples"] == first[1]["acq_samplestamp_samples"] + L == 4 * L
    rc, out = run_selftest(tmp_path, STRONG, 2, ring, 2,
                           extra=["Acquisition_1C.max_dwells=1", "Acquisition_1C.bit_transition_flag=true"])
    assert rc == 0
    check(out, ref, True)
    # and the absent satellite goes negative there
    ref = restatement(ABSENT, 1, 1, True)
    assert [a["event"] for a in ref] == [2]
    rc, out = run_selftest(tmp_path, ABSENT, 1, ring, 1, extra=["Acquisition_1C.bit_transition_flag=true"])
    assert rc == 0
    check(out, ref, True)


def test_state_zero_and_the_event_calls_consume_every_item(tmp_path):
    """Three items offered per call: states 0, 2 and 3 take them all, state 1 takes one."""
    ref = restatement(ABSENT, 1, 3)
    assert [c["consumed"] for c in ref[0]["calls"]] == [3, 1, 1, 3]
    rc, out = run_selftest(tmp_path, ABSENT, 1, 0, per_call=3)
    assert rc == 0
    check(out, ref)


def test_adapter_keys(tmp_path):
    """The default folding factor and the rounding of coherent_integration_time_ms; the pfa threshold
    (per channel, then per role); the two configurations the block refuses."""
    assert qc.default_folding_factor(SPC) == P
    rc, out = run_selftest(tmp_path, ABSENT, 0, ms=6)
    assert rc == 0 and out["sampled_ms"] == qc.sampled_ms_key(6, P) == 4 and out["folding_factor"] == P
    assert np.float32(out["threshold"]) == np.float32(threshold())  # nine printed digits give the float back
    rc, out = run_selftest(tmp_path, ABSENT, 0, ms=3)
    assert rc == 0 and out["sampled_ms"] == qc.sampled_ms_key(3, P) == 4
    want = qc.threshold(0.001, SPC, P, DMAX, DSTEP)
    rc, out = run_selftest(tmp_path, ABSENT, 0, extra=["Acquisition_1C.pfa=0.001"])
    assert rc == 0 and abs(out["threshold"] - want) <= 1e-6 * want, (out["threshold"], want)
    rc, out = run_selftest(tmp_path, ABSENT, 0, extra=["Acquisition_1C0.pfa=0.01", "Acquisition_1C.pfa=0.001"])
    assert abs(out["threshold"] - qc.threshold(0.01, SPC, P, DMAX, DSTEP)) <= 1e-6 * out["threshold"]
    # an explicit folding factor: 2 ms items on a 2000-point grid
    rc, out = run_selftest(tmp_path, ABSENT, 0, ms=2, extra=["Acquisition_1C.folding_factor=2"])
    assert rc == 0 and (out["item_samples"], out["fft_size"], out["folding_factor"]) == (2 * SPC, SPC // 2, 2)
    # the reference's flow graph does not connect: 8 ms items for a block fed 4 ms vectors
    rc, out = run_selftest(tmp_path, ABSENT, 0, ms=8)
    assert rc != 0 and out["built"] is False and "must equal folding_factor" in out["error"]
    # the reference never leaves calculate_threshold's loop with a zero step
    rc, out = run_selftest(tmp_path, ABSENT, 0, step=0, extra=["Acquisition_1C.pfa=0.001"])
    assert rc != 0 and out["configured"] is False and "set_doppler_step" in out["error"]
    # folding factors the block refuses
    for p, ms in ((1, 1), (3, 3), (20, 20)):
        rc, out = run_selftest(tmp_path, ABSENT, 0, ms=ms, extra=["Acquisition_1C.folding_factor=%d" % p])
        assert rc != 0 and out["built"] is False and ("folding" in out["error"]), out

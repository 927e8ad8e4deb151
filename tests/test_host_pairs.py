"""The host mirror of pcps_cccwsr_acquisition_cc and galileo_pcps_8ms_acquisition_cc
(host/pcps_pair_acquisition_mi355x.cc and its two adapters), built by the block factory from a
.conf and driven through its state machine by host/tests/pair_acquisition_selftest.cc with
max_dwells = 2, from a host buffer and from the device ring.

The program reports, for every work() call, the state before it, what it consumed, the event
and the Gnss_Synchro acquisition fields; they are compared call by call with the restatement of
the whole block in tests/pair_checks.py (RefBlock).  Three satellites per stream:
  STRONG  in every item: positive at the first dwell;
  CARRY   only in the items of dwell 0, which are loud (noise power 4): the statistic of dwell 0
          stays under the threshold, and dwell 1 (quiet, the satellite gone) is positive only
          for CCCWSR, whose d_mag survives the dwell -- the 8 ms block goes negative;
  ABSENT  negative after two dwells."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import pair_checks as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "pair_acquisition_selftest")
FS, SPC, DMAX, DSTEP, DWELLS, ITEMS = 4000000, 16000, 1000, 250, 2, 9
STRONG, CARRY, ABSENT = 11, 19, 30
THRESHOLD = 0.02
KEYS = {pc.CCCWSR: "Galileo_E1_PCPS_CCCWSR_Ambiguous_Acquisition_MI355X",
        pc.PCPS_8MS: "Galileo_E1_PCPS_8ms_Ambiguous_Acquisition_MI355X"}


def fft_size(policy):
    return SPC if policy == pc.CCCWSR else 2 * SPC


def replicas(policy, prn):
    """What the adapter's set_local_code hands the block, and what the block makes of it."""
    B, C = pc.codes_for(prn, SPC, SPC)
    if policy == pc.CCCWSR:
        return B, C
    code = np.tile(B, 2)
    return code, pc.members_8ms(code, SPC)[1].astype(np.complex64)


@functools.lru_cache(maxsize=None)
def stream(policy):
    """ITEMS items; items 1, 5, ... (dwell 0 of an attempt that starts at item 0, 4, ...) are loud
    and hold CARRY; STRONG is in every item.  Peaks: mag 0.2 (STRONG) and 0.04 (CARRY)."""
    N = fft_size(policy)
    rows = pc.doppler_rows(DMAX, DSTEP)
    rng = np.random.default_rng(20260 + N)
    x = np.zeros((ITEMS, N), np.complex128)
    for i in range(ITEMS):
        loud = i % 4 == 1
        for prn, amp, row, tau, on in ((STRONG, np.sqrt(0.2), 6, 2920, True), (CARRY, np.sqrt(0.04), 1, 7777, loud)):
            if not on:
                continue
            B, C = (c.astype(np.complex128) for c in pc.codes_for(prn, SPC, SPC))
            if policy == pc.CCCWSR:
                x[i] += pc.member_signal(B, C, tau, 1.0, 1.0 if prn == CARRY else -1.0, rows[row], FS, amp / 2.0, 0,
                                         noise=0.0, n0=i * N)
            else:
                x[i] += pc.bits_signal(B, SPC, tau, (-1, 1, -1) if prn == STRONG else (1, 1, 1), rows[row], FS, amp, 0,
                                       noise=0.0, phase=0.5 * i)
        sigma = 2.0 if loud else 1.0
        x[i] += sigma * (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.5)
    return x.astype(np.complex64).reshape(-1)


@functools.lru_cache(maxsize=None)
def restatement(policy, prn, attempts, per_call=1):
    first, second = replicas(policy, prn)
    blk = pc.RefBlock(policy, FS, fft_size(policy), SPC, DMAX, DSTEP, DWELLS, float(np.float32(THRESHOLD)), first, second)
    return pc.run_attempts(blk, stream(policy), attempts, per_call)


def run_selftest(tmp_path, policy, prn, attempts, ring=0, per_call=1, extra=(), ms=None):
    iq = tmp_path / "iq.dat"
    stream(policy).tofile(iq)
    conf = tmp_path / "pair.conf"
    conf.write_text("\n".join([
        "; paired-code Galileo E1 acquisition on the MI355X engine",
        "[GNSS-SDR]",
        "GNSS-SDR.internal_fs_sps=%d" % FS,
        "Acquisition_1B.implementation=%s" % KEYS[policy],
        "Acquisition_1B.item_type=gr_complex",
        "Acquisition_1B.coherent_integration_time_ms=%d" % (ms if ms is not None else (4 if policy == pc.CCCWSR else 8)),
        "Acquisition_1B.doppler_max=%d" % DMAX,
        "Acquisition_1B.doppler_step=%d" % DSTEP,
        "Acquisition_1B.max_dwells=%d" % DWELLS,
    ] + list(extra)) + "\n")
    r = subprocess.run([EXE, str(conf), str(iq), str(prn), repr(THRESHOLD), str(attempts), str(ring), str(per_call)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def dwell_records(policy, prn, items):
    first, second = replicas(policy, prn)
    N, x = fft_size(policy), stream(policy)
    return [pc.block_record(x[i * N:(i + 1) * N], FS, DMAX, DSTEP, policy, first, second, SPC, i * N) for i in items]


def check(out, ref, policy):
    N = fft_size(policy)
    assert out["built"] and out["implementation"] == KEYS[policy]
    assert (out["fft_size"], out["num_doppler_bins"], out["max_dwells"], out["doppler_max"]) == (N, 9, DWELLS, DMAX)
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
                assert abs(c[k] - r[k]) <= pc.RTOL * abs(r[k]), (k, c, r)


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("policy", [pc.CCCWSR, pc.PCPS_8MS])
@pytest.mark.parametrize("prn", [STRONG, CARRY, ABSENT])
def test_block_against_restatement(tmp_path, prn, policy, ring):
    attempts = 2
    ref = restatement(policy, prn, attempts)
    # every dwell the attempts ran is pinned: row, member and index margins
    N = fft_size(policy)
    for a in ref:
        assert a["event"] in (1, 2)
    items = sorted({1, 2, 5, 6} if prn != STRONG else {1, 4})
    for rec in dwell_records(policy, prn, tuple(items)):
        assert min(rec["margins"].values()) >= pc.MIN_MARGIN, rec["margins"]
    # the three stories
    events = [a["event"] for a in ref]
    dwells = [sum(c["state"] == 1 for c in a["calls"]) for a in ref]
    if prn == STRONG:
        assert events == [1, 1] and dwells == [1, 1]
    elif prn == ABSENT:
        assert events == [2, 2] and dwells == [2, 2]
    else:
        recs = [r["rec"] for r in dwell_records(policy, prn, (1, 2))]
        carry, no_carry = pc.decide(recs, THRESHOLD, True), pc.decide(recs, THRESHOLD, False)
        assert (carry[1], carry[2]) == (True, 2) and (no_carry[1], no_carry[2]) == (False, 2)
        assert events == ([1, 1] if policy == pc.CCCWSR else [2, 2]) and dwells == [2, 2]
        if policy == pc.CCCWSR:
            # published by dwell 1's call, the fields are dwell 0's: the stamp is the end of item 1
            assert ref[0]["calls"][2]["acq_samplestamp_samples"] == 2 * N and ref[0]["calls"][2]["acq_doppler_hz"] == -750.0
    rc, out = run_selftest(tmp_path, policy, prn, attempts, ring)
    assert rc == 0
    check(out, ref, policy)


def test_state_zero_and_the_event_calls_consume_every_item(tmp_path):
    """Three items offered per call: states 0, 2 and 3 take them all, state 1 takes one."""
    ref = restatement(pc.CCCWSR, ABSENT, 1, 3)
    assert [c["consumed"] for c in ref[0]["calls"]] == [3, 1, 1, 3]
    rc, out = run_selftest(tmp_path, pc.CCCWSR, ABSENT, 1, 0, per_call=3)
    assert rc == 0
    check(out, ref, pc.CCCWSR)


def test_adapter_keys(tmp_path):
    """coherent_integration_time_ms is rounded down to a multiple of 4; the 8 ms adapter's pfa
    threshold (per channel, then per role); the 8 ms block refuses one code period per item."""
    rc, out = run_selftest(tmp_path, pc.CCCWSR, ABSENT, 0, ms=7, extra=["Acquisition_1B.pfa=0.5"])
    assert rc == 0 and out["sampled_ms"] == pc.sampled_ms_key(7) == 4 and out["fft_size"] == SPC
    # CCCWSR has no pfa threshold (nine printed digits give the float back)
    assert np.float32(out["threshold"]) == np.float32(THRESHOLD)
    want = pc.threshold_8ms(0.001, 2 * SPC, DMAX, DSTEP)
    rc, out = run_selftest(tmp_path, pc.PCPS_8MS, ABSENT, 0, ms=11, extra=["Acquisition_1B.pfa=0.001"])
    assert rc == 0 and out["sampled_ms"] == 8 and out["fft_size"] == 2 * SPC
    assert abs(out["threshold"] - want) <= 1e-6 * want, (out["threshold"], want)
    rc, out = run_selftest(tmp_path, pc.PCPS_8MS, ABSENT, 0, ms=8,
                           extra=["Acquisition_1B0.pfa=0.01", "Acquisition_1B.pfa=0.001"])
    assert abs(out["threshold"] - pc.threshold_8ms(0.01, 2 * SPC, DMAX, DSTEP)) <= 1e-6 * out["threshold"]
    rc, out = run_selftest(tmp_path, pc.PCPS_8MS, ABSENT, 0, ms=4)
    assert rc != 0 and out["built"] is False and "coherent_integration_time_ms >= 8" in out["error"]

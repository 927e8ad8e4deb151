"""The host mirror of pcps_tong_acquisition_cc (host/pcps_tong_acquisition_mi355x.cc and its adapters
host/gps_l1_ca_pcps_tong_acquisition_mi355x.cc and
host/galileo_e1_pcps_tong_ambiguous_acquisition_mi355x.cc), built by the block factory from a .conf
and driven through its state machine by host/tests/tong_acquisition_selftest.cc, from a host buffer
and from the device ring.

Shapes: GPS L1 C/A at 4 Msps with 1 ms items (4000 samples) and Galileo E1 at 4 Msps with 4 ms items
(16000 samples, the running row in HBM), +-1000 Hz / 250 Hz, tong_init_val 2, tong_max_val 4,
tong_max_dwells 8.  The program reports, for every work() call, the state before it, what it
consumed, the event, the counters, the Gnss_Synchro acquisition fields and the monitor output; they
are compared call by call with the restatement of the whole block in tests/tong_checks.py (RefBlock;
with several items offered per call, RefBlock's batch mode: as many reference calls in one).
  STRONG  in every item: two dwells up, positive;
  ABSENT  two dwells down, negative.
The threshold is chosen on the CPU from the restatement's statistic of every item on its own (an
item's share of any dwell's accumulated statistic): the geometric mean of ABSENT's largest and
STRONG's smallest, which must lie a factor 2 from both."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from gsdr import synth

import tong_checks as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "tong_acquisition_selftest")
FS, DMAX, DSTEP, ITEMS = 4000000, 1000, 250, 16
INIT, TMAX, MAXD = 2, 4, 8
STRONG, ABSENT = 11, 30
SYSTEMS = {
    "gps": dict(role="Acquisition_1C", key="GPS_L1_CA_PCPS_Tong_Acquisition_MI355X", n=4000, ms=1, code_length=4000,
                delay=2921),
    "gal": dict(role="Acquisition_1B", key="Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_MI355X", n=16000, ms=4,
                code_length=16000, delay=12921),
}


@functools.lru_cache(maxsize=None)
def code(system, prn):
    c = synth.gps_ca_sampled(prn, FS) if system == "gps" else synth.gal_e1_sampled(prn, FS)
    assert len(c) == SYSTEMS[system]["n"]
    return np.asarray(c).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def stream(system):
    """ITEMS items with STRONG in each (row 6 = 500 Hz)."""
    s = SYSTEMS[system]
    rows = tc.doppler_rows(DMAX, DSTEP)
    rng = np.random.default_rng(synth.SEED + 9500 + s["n"])
    n = np.arange(ITEMS * s["n"])
    c = code(system, STRONG).astype(np.complex128)[(n - s["delay"]) % s["n"]]
    x = np.sqrt(0.05) * c * np.exp(1j * (2 * np.pi * rows[6] * n / FS + 0.3))
    x = x + (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n))) * np.sqrt(0.5)
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def item_statistics(system, prn):
    """Every item on its own: (statistic, winner margin)."""
    s = SYSTEMS[system]
    x = stream(system).astype(np.complex128)
    rows = tc.doppler_rows(DMAX, DSTEP)
    out = []
    for i in range(ITEMS):
        w = tc.winner(tc.item_rows(x[i * s["n"]:(i + 1) * s["n"]], FS, rows, code(system, prn)))
        out.append((w[2], w[3]))
    return out


@functools.lru_cache(maxsize=None)
def threshold(system):
    strong = min(m for m, _ in item_statistics(system, STRONG))
    absent = max(m for m, _ in item_statistics(system, ABSENT))
    thr = float(np.float32(np.sqrt(strong * absent)))
    assert absent * 2.0 <= thr <= strong / 2.0, (absent, thr, strong)
    return thr


@functools.lru_cache(maxsize=None)
def restatement(system, prn, attempts, per_call=1, monitor=False, init=INIT, tmax=TMAX, maxd=MAXD):
    s = SYSTEMS[system]
    blk = tc.RefBlock(FS, s["n"], s["code_length"], DMAX, DSTEP, threshold(system), init, tmax, maxd,
                      code=code(system, prn), monitor=monitor, batch=min(maxd, 32))
    return tc.run_attempts(blk, stream(system).astype(np.complex128), attempts, per_call)


def run_selftest(tmp_path, system, prn, attempts, ring=0, per_call=1, extra=(), ms=None, thr=None, step=DSTEP,
                 tong=(INIT, TMAX, MAXD)):
    s = SYSTEMS[system]
    role = s["role"]
    iq = tmp_path / "iq.dat"
    stream(system).tofile(iq)
    conf = tmp_path / "tong.conf"
    lines = [
        "; Tong acquisition on the MI355X engine",
        "[GNSS-SDR]",
        "GNSS-SDR.internal_fs_sps=%d" % FS,
        "%s.implementation=%s" % (role, s["key"]),
        "%s.item_type=gr_complex" % role,
        "%s.coherent_integration_time_ms=%d" % (role, s["ms"] if ms is None else ms),
        "%s.doppler_max=%d" % (role, DMAX),
        "%s.doppler_step=%d" % (role, step),
    ]
    if tong is not None:
        lines += ["%s.tong_init_val=%d" % (role, tong[0]), "%s.tong_max_val=%d" % (role, tong[1]),
                  "%s.tong_max_dwells=%d" % (role, tong[2])]
    conf.write_text("\n".join(lines + list(extra)) + "\n")
    thr = threshold(system) if thr is None else thr
    r = subprocess.run([EXE, str(conf), str(iq), role, str(prn), repr(thr), str(attempts), str(ring), str(per_call)],
                       capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def check(system, out, ref, tong=(INIT, TMAX, MAXD)):
    s = SYSTEMS[system]
    assert out["built"] and out["implementation"] == s["key"]
    assert (out["item_samples"], out["vector_length"], out["code_length"], out["num_doppler_bins"], out["doppler_max"],
            out["sampled_ms"]) == (s["n"], s["n"], s["code_length"], 9, DMAX, s["ms"])
    assert (out["tong_init_val"], out["tong_max_val"], out["tong_max_dwells"]) == tong
    assert len(out["attempts"]) == len(ref)
    for a, w in zip(out["attempts"], ref):
        for k in ("state", "offered", "consumed", "event", "dwell_count", "tong_count"):
            assert [c[k] for c in a["calls"]] == [c[k] for c in w["calls"]], k
        assert (a["event"], a["end_state"], a["sample_counter"]) == (w["event"], w["end_state"], w["sample_counter"])
        for c, r in zip(a["calls"], w["calls"]):
            assert c["acq_delay_samples"] == r["acq_delay_samples"], (c, r)
            assert c["acq_doppler_hz"] == r["acq_doppler_hz"], (c, r)
            assert c["acq_samplestamp_samples"] == r["acq_samplestamp_samples"], (c, r)  # the end of the item
            assert c["acq_doppler_step"] == r["acq_doppler_step"], (c, r)
            for k in ("mag", "input_power"):
                assert abs(c[k] - r[k]) <= tc.RTOL * abs(r[k]), (k, c, r)
            if r["monitor"] is None:
                assert c["monitor"] is None, (c, r)
            else:
                assert {k: c["monitor"][k] for k in r["monitor"]} == r["monitor"], (c, r)


def _pin_margins(system, ref):
    """The winner behind every state-1 call of the restated attempts 1e-3 above its runner-up, and its
    statistic 5 % from threshold * dwell."""
    thr = threshold(system)
    for a in ref:
        for c in a["calls"]:
            if c["state"] == 1:
                assert c["winner_margin"] >= tc.MIN_MARGIN, c
                assert abs(c["mag"] - thr * c["dwell_count"]) >= tc.MIN_DECISION * thr * c["dwell_count"], c


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("prn", [STRONG, ABSENT])
@pytest.mark.parametrize("system", ["gps", "gal"])
def test_block_against_restatement(tmp_path, system, prn, ring):
    """Two attempts, three items offered per call, the monitor output enabled."""
    s = SYSTEMS[system]
    attempts, per_call = 2, 3
    ref = restatement(system, prn, attempts, per_call, True)
    _pin_margins(system, ref)
    events = [a["event"] for a in ref]
    calls = ref[0]["calls"]
    # state 0 takes the three items offered; the next call offers three, and the sequence ends on its second
    assert [(c["state"], c["consumed"]) for c in calls] == [(0, 3), (1, 2), (2 if prn == STRONG else 3, 3)]
    if prn == STRONG:
        assert events == [1, 1]
        assert (calls[1]["acq_delay_samples"], calls[1]["acq_doppler_hz"], calls[1]["acq_samplestamp_samples"]) == \
            (float(s["delay"] % s["code_length"]), 500.0, 5 * s["n"])
        assert calls[2]["monitor"]["acq_samplestamp_samples"] == 5 * s["n"]
    else:
        assert events == [2, 2] and all(c["monitor"] is None for c in calls)
    rc, out = run_selftest(tmp_path, system, prn, attempts, ring, per_call,
                           extra=["AcquisitionMonitor.enable_monitor=true"])
    assert rc == 0
    check(system, out, ref)


@pytest.mark.parametrize("system", ["gps", "gal"])
def test_one_item_per_call_is_the_reference_call_for_call(tmp_path, system):
    """One item offered per call: the reference's own sequence of calls (RefBlock consumes one item per
    state-1 call whatever its batch), without the monitor output."""
    for prn in (STRONG, ABSENT):
        ref = restatement(system, prn, 2, 1)
        _pin_margins(system, ref)
        assert [(c["state"], c["consumed"]) for c in ref[0]["calls"]] == \
            [(0, 1), (1, 1), (1, 1), (2 if prn == STRONG else 3, 1)]
        rc, out = run_selftest(tmp_path, system, prn, 2, 0, 1)
        assert rc == 0
        check(system, out, ref)
        assert all(c["monitor"] is None for a in out["attempts"] for c in a["calls"])


def test_adapter_keys(tmp_path):
    """The defaults of the counter (1, 2, tong_max_val + 1), the pfa threshold (per channel, then per
    role), Galileo's rounding of coherent_integration_time_ms, and the counters the block refuses."""
    ref = restatement("gps", STRONG, 1, 1, False, 1, 2, 3)
    _pin_margins("gps", ref)
    assert [(c["state"], c["consumed"]) for c in ref[0]["calls"]] == [(0, 1), (1, 1), (2, 1)]  # one dwell decides
    rc, out = run_selftest(tmp_path, "gps", STRONG, 1, tong=None)
    assert rc == 0
    check("gps", out, ref, (1, 2, 3))
    assert np.float32(out["threshold"]) == np.float32(threshold("gps"))  # nine printed digits give the float back
    rc, out = run_selftest(tmp_path, "gps", ABSENT, 0, tong=None, extra=["Acquisition_1C.tong_max_val=5"])
    assert rc == 0 and (out["tong_init_val"], out["tong_max_val"], out["tong_max_dwells"]) == (1, 5, 6)
    want = tc.threshold(0.001, 4000, 9)
    rc, out = run_selftest(tmp_path, "gps", ABSENT, 0, extra=["Acquisition_1C.pfa=0.001"])
    assert rc == 0 and abs(out["threshold"] - want) <= 1e-6 * want, (out["threshold"], want)
    rc, out = run_selftest(tmp_path, "gps", ABSENT, 0, extra=["Acquisition_1C0.pfa=0.01", "Acquisition_1C.pfa=0.001"])
    assert abs(out["threshold"] - tc.threshold(0.01, 4000, 9)) <= 1e-6 * out["threshold"]
    # two code periods per item: lambda and the cell count follow the vector length
    rc, out = run_selftest(tmp_path, "gps", ABSENT, 0, ms=2, extra=["Acquisition_1C.pfa=0.001"])
    assert rc == 0 and (out["item_samples"], out["vector_length"], out["code_length"]) == (8000, 8000, 4000)
    assert abs(out["threshold"] - tc.threshold(0.001, 8000, 9)) <= 1e-6 * out["threshold"]
    rc, out = run_selftest(tmp_path, "gal", ABSENT, 0, ms=7, extra=["Acquisition_1B.pfa=0.001"])
    assert rc == 0 and (out["sampled_ms"], out["item_samples"]) == (4, 16000)
    assert abs(out["threshold"] - tc.threshold(0.001, 16000, 9)) <= 1e-6 * out["threshold"]
    # counters the reference cannot run, and the zero Doppler step its loops never leave
    for tong in ((0, 2, 3), (2, 2, 3), (1, 2, 0)):
        rc, out = run_selftest(tmp_path, "gps", ABSENT, 0, tong=tong)
        assert rc != 0 and out["built"] is False and "tong" in out["error"], out
    rc, out = run_selftest(tmp_path, "gps", ABSENT, 0, step=0)
    assert rc != 0 and out["configured"] is False and "set_doppler_step" in out["error"]
    rc, out = run_selftest(tmp_path, "gal", ABSENT, 0, ms=3)
    assert rc != 0 and out["built"] is False  # 3 ms round down to no item at all

"""The host mirror of galileo_e5a_noncoherentIQ_acquisition_caf_cc
(host/galileo_e5a_noncoherent_iq_acquisition_caf_block_mi355x.cc and its adapter
host/galileo_e5a_noncoherent_iq_acquisition_caf_mi355x.cc), built by the block factory from a .conf
with a temporary random code table and driven through its state machine by
host/tests/iq_caf_acquisition_selftest.cc, from a host buffer and from the device ring.

Shapes: 4 Msps (4000 samples per code), +-1000 Hz / 250 Hz; 1 ms items of 4000 samples, 2 ms items of
8000, and the zero-padded form (8000: 1 ms of code and 1 ms of zeros).  The stream holds PRN STRONG on
both components throughout, at 0.8 of its amplitude in every second stretch of 8000 samples, so
that with bit_transition_flag the weaker second dwell does not take over.  The program reports, for
every work() call, the state before it, what it consumed, the event, the dwell count and statistic,
the Gnss_Synchro acquisition fields and the monitor output; they are compared call by call with the
restatement of the whole block in tests/iq_caf_checks.py (RefBlock; with several items offered per
call, RefBlock's batch mode: as many reference dwells in one).
The threshold is chosen on the CPU from the restatement's statistic of every item on its own: the
geometric mean of ABSENT's largest and STRONG's smallest, which must lie a factor 2 from both."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from gsdr import synth

import iq_caf_checks as qc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "iq_caf_acquisition_selftest")
KEY = "Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_MI355X"
ROLE = "Acquisition_5X"
FS, SPC, DMAX, DSTEP, SAMPLES = 4000000, 4000, 1000, 250, 16 * 8000
STRONG, ABSENT, ROW, DELAY = 11, 30, 6, 2921
STREAM_SEED = 3  # the first for which the dwells of every test below meet their margins
# name: (coherent_integration_time_ms, Zero_padding, max_dwells, bit_transition_flag, CAF_window_hz)
SHAPES = {"1ms": (1, 0, 2, False, 0), "2ms": (2, 0, 2, False, 0), "zp": (1, 1, 2, False, 0),
          "bt_caf": (2, 0, 2, True, 1000)}


@functools.lru_cache(maxsize=None)
def table():
    return qc.e5a_random_table(515)


@functools.lru_cache(maxsize=None)
def stream():
    """STRONG in every sample (row 6 = 500 Hz); stretches 0, 2, ... of 8000 samples at 0.8 of the amplitude."""
    rng = np.random.default_rng(synth.SEED + 9700 + STREAM_SEED)
    n = np.arange(SAMPLES)
    ci = qc.e5a_sampled(table(), STRONG, "5I", FS).real.astype(np.float64)
    cq = qc.e5a_sampled(table(), STRONG, "5Q", FS).real.astype(np.float64)
    ph = (n - DELAY) % SPC
    amp = np.where((n // 8000) % 2 == 0, 0.8, 1.0) * 0.15
    rows = qc.doppler_rows(DMAX, DSTEP)
    x = amp * (ci[ph] + 1j * cq[ph]) * np.exp(1j * (2 * np.pi * rows[ROW] * n / FS + 0.3))
    x = x + (rng.standard_normal(SAMPLES) + 1j * rng.standard_normal(SAMPLES)) * np.sqrt(0.5)
    return x.astype(np.complex64)


def _shape(name):
    ms, zp, maxd, bt, window = SHAPES[name]
    vec_ms = 2 if zp else ms
    return dict(ms=ms, zp=zp, maxd=maxd, bt=bt, window=window, n=vec_ms * SPC, block_ms=1 if zp else vec_ms)


@functools.lru_cache(maxsize=None)
def forms(name, prn):
    s = _shape(name)
    ci = qc.e5a_sampled(table(), prn, "5I", FS)
    cq = qc.e5a_sampled(table(), prn, "5Q", FS)
    return qc.forms(qc.tiled(ci, s["block_ms"], s["n"]), qc.tiled(cq, s["block_ms"], s["n"]), SPC, s["block_ms"], True)


@functools.lru_cache(maxsize=None)
def item_records(name, prn):
    """Every item on its own -> the restatement's records (with their margins)."""
    s = _shape(name)
    x = stream().astype(np.complex128)
    return [qc.item_record(x[i * s["n"]:(i + 1) * s["n"]], FS, DMAX, DSTEP, forms(name, prn), SPC, s["window"])
            for i in range(SAMPLES // s["n"])]


@functools.lru_cache(maxsize=None)
def threshold(name):
    strong = min(r["test_statistic"] for r, _ in item_records(name, STRONG))
    absent = max(r["test_statistic"] for r, _ in item_records(name, ABSENT))
    thr = float(np.float32(np.sqrt(strong * absent)))
    assert absent * 2.0 <= thr <= strong / 2.0, (absent, thr, strong)
    return thr


def _pin_margins(name, ref):
    """Every margin of every dwell of the restated attempts, and the deciding statistics 5 % from the
    threshold (iq_caf_checks.assert_attempt_margins)."""
    qc.assert_attempt_margins(ref, threshold(name))


@functools.lru_cache(maxsize=None)
def restatement(name, prn, attempts, per_call=1, monitor=False):
    s = _shape(name)
    blk = qc.RefBlock(FS, s["n"], SPC, DMAX, DSTEP, threshold(name), s["maxd"], s["bt"], fm=forms(name, prn),
                      window_hz=s["window"], monitor=monitor, batch=min(s["maxd"], 32))
    return qc.run_attempts(blk, stream().astype(np.complex128), attempts, per_call)


def run_selftest(tmp_path, name, prn, attempts, ring=0, per_call=1, extra=(), with_table=True, env_table=False,
                 thr=None, signal="5X"):
    s = _shape(name)
    iq = tmp_path / "iq.dat"
    stream().tofile(iq)
    codes = tmp_path / "e5a_codes.bin"
    codes.write_bytes(table())
    conf = tmp_path / "iq_caf.conf"
    lines = [
        "; E5a non-coherent IQ acquisition with CAF filter on the MI355X engine",
        "[GNSS-SDR]",
        "GNSS-SDR.internal_fs_sps=%d" % FS,
        "Channel.signal=%s" % signal,
        "%s.implementation=%s" % (ROLE, KEY),
        "%s.item_type=gr_complex" % ROLE,
        "%s.coherent_integration_time_ms=%d" % (ROLE, s["ms"]),
        "%s.Zero_padding=%d" % (ROLE, s["zp"]),
        "%s.max_dwells=%d" % (ROLE, s["maxd"]),
        "%s.bit_transition_flag=%s" % (ROLE, "true" if s["bt"] else "false"),
        "%s.CAF_window_hz=%d" % (ROLE, s["window"]),
        "%s.doppler_max=%d" % (ROLE, DMAX),
        "%s.doppler_step=%d" % (ROLE, DSTEP),
    ]
    if with_table and not env_table:
        lines.append("%s.e5a_code_table=%s" % (ROLE, codes))
    conf.write_text("\n".join(lines + list(extra)) + "\n")
    env = dict(os.environ)
    env.pop("GSDR_GALILEO_E5A_CODES", None)
    if env_table:
        env["GSDR_GALILEO_E5A_CODES"] = str(codes)
    thr = threshold(name) if thr is None else thr
    r = subprocess.run([EXE, str(conf), str(iq), ROLE, str(prn), repr(thr), str(attempts), str(ring), str(per_call)],
                       capture_output=True, text=True, timeout=120, env=env)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r.returncode, json.loads(r.stdout.strip().splitlines()[-1])


def check(name, out, ref):
    s = _shape(name)
    assert out["built"] and out["implementation"] == KEY
    assert (out["item_samples"], out["vector_length"], out["code_length"], out["num_doppler_bins"], out["doppler_max"]) == \
        (s["n"], s["n"], SPC, 9, DMAX)
    assert (out["sampled_ms"], out["coherent_ms"], out["max_dwells"], out["caf_window_hz"], out["zero_padding"],
            out["bit_transition_flag"], out["both_components"]) == \
        (s["n"] // SPC, s["block_ms"], s["maxd"], s["window"], s["zp"], s["bt"], True)
    assert len(out["attempts"]) == len(ref)
    for a, w in zip(out["attempts"], ref):
        for k in ("state", "offered", "consumed", "event", "well_count"):
            assert [c[k] for c in a["calls"]] == [c[k] for c in w["calls"]], k
        assert (a["event"], a["end_state"], a["sample_counter"]) == (w["event"], w["end_state"], w["sample_counter"])
        for c, r in zip(a["calls"], w["calls"]):
            assert c["acq_delay_samples"] == r["acq_delay_samples"], (c, r)
            assert c["acq_doppler_hz"] == r["acq_doppler_hz"], (c, r)
            assert c["acq_samplestamp_samples"] == r["acq_samplestamp_samples"], (c, r)  # the end of the item
            assert c["acq_doppler_step"] == r["acq_doppler_step"], (c, r)
            for k in ("mag", "input_power", "test_statistics"):
                if r[k] == 0.0:
                    assert c[k] == 0.0, (k, c, r)
                else:
                    assert abs(c[k] - r[k]) <= qc.RTOL * abs(r[k]), (k, c, r)
            if r["monitor"] is None:
                assert c["monitor"] is None, (c, r)
            else:
                assert {k: c["monitor"][k] for k in r["monitor"]} == r["monitor"], (c, r)


@pytest.mark.parametrize("ring", [0, 1])
@pytest.mark.parametrize("prn", [STRONG, ABSENT])
@pytest.mark.parametrize("name", ["1ms", "2ms", "zp"])
def test_block_against_restatement(tmp_path, name, prn, ring):
    """Two attempts, three items offered per call, the monitor output enabled: positive after
    max_dwells = 2 for the present satellite, negative for the absent one."""
    s = _shape(name)
    attempts, per_call = 2, 3
    ref = restatement(name, prn, attempts, per_call, True)
    _pin_margins(name, ref)
    calls = ref[0]["calls"]
    # state 0 takes the three items offered; the next call offers three and the attempt takes its two dwells
    assert [(c["state"], c["consumed"]) for c in calls] == [(0, 3), (1, 2), (3 if prn == STRONG else 4, 3)]
    if prn == STRONG:
        assert [a["event"] for a in ref] == [1, 1]
        assert (calls[1]["acq_delay_samples"], calls[1]["acq_doppler_hz"], calls[1]["acq_samplestamp_samples"]) == \
            (float(DELAY), 500.0, 5 * s["n"])
        assert calls[2]["monitor"]["acq_samplestamp_samples"] == 5 * s["n"]
    else:
        assert [a["event"] for a in ref] == [2, 2] and all(c["monitor"] is None for c in calls)
    rc, out = run_selftest(tmp_path, name, prn, attempts, ring, per_call,
                           extra=["AcquisitionMonitor.enable_monitor=true"])
    assert rc == 0
    check(name, out, ref)


@pytest.mark.parametrize("ring", [0, 1])
def test_bit_transition_with_caf(tmp_path, ring):
    """bit_transition_flag with the filter: the weaker second dwell does not take over the delay and the
    stamp, and its CAF Doppler overwrites Acq_doppler_hz all the same; one item per call."""
    name = "bt_caf"
    s = _shape(name)
    ref = restatement(name, STRONG, 2, 1)
    _pin_margins(name, ref)
    calls = ref[0]["calls"]
    assert [(c["state"], c["consumed"]) for c in calls] == [(0, 1), (1, 1), (1, 1), (3, 1)]
    first, second = item_records(name, STRONG)[1][0], item_records(name, STRONG)[2][0]
    assert second["test_statistic"] < first["test_statistic"]
    assert calls[2]["acq_samplestamp_samples"] == calls[1]["acq_samplestamp_samples"] == 2 * s["n"]
    assert calls[2]["test_statistics"] == calls[1]["test_statistics"]
    assert calls[2]["acq_doppler_hz"] == float(second["caf_doppler_hz"])
    # the filter's answer is not the grid's here (the weights of :614 and :634 lean to the lower rows)
    assert second["caf_doppler_hz"] != second["doppler_hz"]
    rc, out = run_selftest(tmp_path, name, STRONG, 2, ring, 1)
    assert rc == 0
    check(name, out, ref)
    assert all(c["monitor"] is None for a in out["attempts"] for c in a["calls"])


def test_adapter_keys_and_code_table(tmp_path):
    """The cap of coherent_integration_time_ms, the pfa threshold (per channel, then per role), the
    table named by the environment, one component, and the refusals: no table, an unreadable one, one
    of the wrong size, and the windows the reference cannot run."""
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, extra=["%s.coherent_integration_time_ms=7" % ROLE])
    assert rc == 0 and (out["sampled_ms"], out["item_samples"], out["coherent_ms"]) == (3, 12000, 3)
    want = qc.threshold(0.001, 12000, DMAX, DSTEP)
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0,
                           extra=["%s.coherent_integration_time_ms=3" % ROLE, "%s.pfa=0.001" % ROLE])
    assert rc == 0 and abs(out["threshold"] - want) <= 1e-6 * want, (out["threshold"], want)
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, extra=["%s0.pfa=0.01" % ROLE, "%s.pfa=0.001" % ROLE])
    assert abs(out["threshold"] - qc.threshold(0.01, 4000, DMAX, DSTEP)) <= 1e-6 * out["threshold"]
    rc, out = run_selftest(tmp_path, "zp", ABSENT, 0, extra=["%s.pfa=0.001" % ROLE])
    assert rc == 0 and (out["sampled_ms"], out["coherent_ms"], out["item_samples"]) == (2, 1, 8000)
    assert abs(out["threshold"] - qc.threshold(0.001, 8000, DMAX, DSTEP)) <= 1e-6 * out["threshold"]
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0)
    assert np.float32(out["threshold"]) == np.float32(threshold("1ms"))  # nine printed digits give the float back
    # the table named by the environment instead of the role's key
    ref = restatement("1ms", STRONG, 1, 1)
    rc, out = run_selftest(tmp_path, "1ms", STRONG, 1, env_table=True)
    assert rc == 0
    check("1ms", out, ref)
    # Channel.signal other than 5X: one component
    rc, out = run_selftest(tmp_path, "2ms", ABSENT, 0, signal="5I")
    assert rc == 0 and out["both_components"] is False
    # no table, a file that is not there, a file of the wrong size
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, with_table=False)
    assert rc != 0 and out["built"] is False and "e5a_code_table" in out["error"] and "not shipped" in out["error"]
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, with_table=False,
                           extra=["%s.e5a_code_table=%s" % (ROLE, tmp_path / "absent.bin")])
    assert rc != 0 and out["built"] is False and "cannot be read" in out["error"]
    short = tmp_path / "short.bin"
    short.write_bytes(table()[:1000])
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, with_table=False,
                           extra=["%s.e5a_code_table=%s" % (ROLE, short)])
    assert rc != 0 and out["built"] is False and "1000 bytes" in out["error"]
    # CAF_bins_half 0 (:605 divides by it), and a window wider than the grid
    for window in (2 * DSTEP - 1, 2 * DSTEP * 5):
        rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, extra=["%s.CAF_window_hz=%d" % (ROLE, window)])
        assert rc != 0 and out["configured"] is False, out
    rc, out = run_selftest(tmp_path, "1ms", ABSENT, 0, extra=["%s.max_dwells=0" % ROLE])
    assert rc != 0 and out["built"] is False and "max_dwells" in out["error"]

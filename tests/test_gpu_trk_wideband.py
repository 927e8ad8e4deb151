"""Galileo E5a (5X) and GPS L5 in the device-resident DLL/PLL loop, pilot and data tracking.

oracle/trk_oracle.c stops at BeiDou B1I, so the loop reference is tests/trk_restatement.py
(pinned against that oracle by test_trk_restatement.py); the correlator reference is the
oracle's VOLK multicorrelator as for every other signal.  Per case, as in test_gpu_trk.py:
every call's taps and data prompt against the correlator fed with the NCO state the GPU
carried into the call (trk_checks._open_loop_sig and its bars), and the restatement's loop
replayed on the GPU's taps (trk_checks._replay_check: exact schedule, states, flags and
prompts, the float fields to its tolerances).  Scenarios: trk_wideband_checks.py.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import gsdr
from gsdr import synth

import trk_wideband_checks as wb
from trk_checks import _conf_sig, _open_loop_sig, _replay_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPL = [-0.25, 0.0, 0.25]


def _start(t, ch, c):
    return t.start(ch, c.prn, c.code, c.delay, c.dop, 0, 0, data_code=c.data_code, secondary_code=c.secondary)


def _run(c, calls, item=gsdr.ITEM_GR_COMPLEX, host=None):
    t = gsdr.Tracking(c.conf(1, item))
    assert _start(t, 0, c) == c.first
    rec, n = t.run(c.iq if host is None else host, 0, calls)
    t.close()
    return rec[0][:n[0]]


def _open_loop(g, c, iq=None):
    return _open_loop_sig(g, c.iq if iq is None else iq, c.code, c.data_code, c.fs, c.dop, EPL, 1, wb.CHIP_RATE, c.vl, 1)


def _prompts_from_taps(g, c):
    """prompt_i / prompt_q of every valid output from d_P_data_accu rebuilt out of the
    records' own taps / data prompts: zero at bit synchronisation and after each output,
    one float accumulation per call (save_correlation_results, :1288-1400), the data
    secondary code wiped in pilot tracking, then the swap where d_interchange_iq is on (tracking)."""
    f32 = np.float32
    sec = {"5X": synth.GAL_E5A_I_SECONDARY, "L5": synth.GPS_L5I_NH}[c.system] if c.pilot else None
    acc, k, want = [f32(0), f32(0)], 0, {}
    for e in range(c.sync_call + 1, len(g)):
        pd = g["data_prompt"][e] if c.pilot else g["taps"][e][2:4]
        sg = f32(-1.0) if (sec is not None and sec[k % len(sec)] == "1") else f32(1.0)
        acc = [f32(acc[0] + pd[0]), f32(acc[1] + pd[1])] if sg > 0 else [f32(acc[0] - pd[0]), f32(acc[1] - pd[1])]
        k += 1
        if k % c.spb == 0:
            want[e] = (float(acc[1]), float(acc[0])) if c.swap else (float(acc[0]), float(acc[1]))
            acc = [f32(0), f32(0)]
    return want


def _check_case(g, c, open_loop_calls=None):
    assert np.all(np.diff(g["sample_counter"].astype(np.int64)) == g["consumed"][:-1]), c.tag
    if open_loop_calls is None:
        assert _open_loop(g, c) <= 1e-4, c.tag
    else:
        for sl in open_loop_calls:
            assert _open_loop_at(g, c, sl) <= 1e-4, (c.tag, sl)
    _replay_check(g, c.restatement()[0], c.tag)
    wb.check_locked_run(g, c)
    want = _prompts_from_taps(g, c)
    out = np.nonzero(g["flags"] & gsdr.TRK_F_VALID_OUTPUT)[0]
    assert list(out) == sorted(want), c.tag
    for e in out:
        assert (g["prompt_i"][e], g["prompt_q"][e]) == want[e], (c.tag, e)


def _open_loop_at(g, c, sl):
    """_open_loop on the calls of slice sl.  The check takes a call's NCO state from the
    record before it (call 0's from the acquisition), so a slice that starts later is
    preceded by call 0, call 1 (checked like any other) and, as the carrier of the state
    the slice's first call started from, the loop-state fields of the record before the
    slice written into that copy of call 1."""
    if sl.start == 0:
        return _open_loop(g[sl], c)
    bridge = g[1:2].copy()
    for f in ("rem_carr_phase_rad", "carrier_doppler_hz", "rem_code_phase_samples", "code_freq_chips"):
        bridge[f] = g[sl.start - 1][f]
    return _open_loop(np.concatenate([g[0:1], bridge, g[sl]]), c)


@pytest.mark.parametrize("system,pilot", wb.CASES)
def test_loop_parity_staged_window(system, pilot):
    """fs = 4e6: calls of 4000 samples (<= the staged window), a code step of 2.56 chips
    per sample, 1.3 s through pull-in, bit synchronisation and state 4."""
    c = wb.case(system, pilot)
    _check_case(_run(c, 1400), c)


def test_e5a_pilot_streamed_path():
    """fs = 5e6: calls of 5000 samples, one full chunk and a tail through the LDS stream buffers."""
    c = wb.case("5X", 1, 5.0e6)
    g = _run(c, 1400)
    s = c.sync_call
    _check_case(g, c, [slice(0, 64), slice(s - 32, s + 32), slice(len(g) - 64, len(g))])


@functools.lru_cache(maxsize=None)
def _case_24():
    return wb.Case("5X", 1, 24.0e6, seconds=0.052)


@pytest.mark.parametrize("item", [gsdr.ITEM_GR_COMPLEX, gsdr.ITEM_CSHORT])
def test_e5a_pilot_at_24_msps(item):
    """The shape whose two float replicas did not fit the LDS next to the stream buffers:
    24000-sample calls, 48 of them from the start (state 2)."""
    c = _case_24()
    if item == gsdr.ITEM_CSHORT:
        host = synth.to_cshort(c.iq, 800.0)
        ref = (host[0::2].astype(np.float32) + 1j * host[1::2].astype(np.float32)).astype(np.complex64)
    else:
        host, ref = c.iq, c.iq
    g = _run(c, 48, item, host)
    assert len(g) == 48 and np.all(g["state"] == 2)
    assert _open_loop(g, c, ref) <= 1e-4
    _replay_check(g, c.restatement()[0], c.tag)


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import gsdr
from trk_checks import _conf_sig
from gsdr import synth
iq = np.load(sys.argv[1])
t = gsdr.Tracking(_conf_sig(4.0e6, gsdr.SIGNAL_GAL_1B, 2, 1))
for ch, (prn, delay) in enumerate(((11, float(sys.argv[3])), (19, float(sys.argv[4])))):
    t.start(ch, prn, synth.gal_e1_sinboc11(prn, pilot=True), delay, 1250.0, 0, 0, data_code=synth.gal_e1_sinboc11(prn))
rec, n = t.run(iq, 0, 400)
np.savez(sys.argv[2], rec=rec, n=n)
"""


def test_compact_layout_equals_float_layout_on_galileo_e1(tmp_path):
    """Galileo E1 pilot tracking (the scenario of test_gpu_trk.py, two channels) with and
    without GSDR_TRK_PACK_REPLICAS=1, each in a fresh process: byte-equal records."""
    fs = 4.0e6
    sats = [synth.GalileoSatellite(11, 1234.5, 1000.3, 50.0, 0.7), synth.GalileoSatellite(19, 1262.0, 2500.6, 48.0, 1.9)]
    iq = synth.gal_e1_iq(fs, int(1.5 * fs), sats, seed_offset=5)
    delays = [float(round(s.code_delay_chips / (1.023e6 * (1 + s.doppler_hz / 1.57542e9)) * fs) % 16000) for s in sats]
    np.save(tmp_path / "iq.npy", iq)
    recs = []
    for pack in ("0", "1"):
        env = dict(os.environ, GSDR_TRK_PACK_REPLICAS=pack)
        if pack == "0":
            del env["GSDR_TRK_PACK_REPLICAS"]
        out = tmp_path / ("rec%s.npz" % pack)
        subprocess.run([sys.executable, "-c", _CHILD % (os.path.join(ROOT, "gnss-sdr-new_amd"), os.path.join(ROOT, "tests")),
                        str(tmp_path / "iq.npy"), str(out), str(delays[0]), str(delays[1])], check=True, timeout=120,
                       cwd=ROOT)
        recs.append(np.load(out))
    n = recs[0]["n"]
    assert list(n) == list(recs[1]["n"]) and min(n) >= 370, (n, recs[1]["n"])
    assert recs[0]["rec"].tobytes() == recs[1]["rec"].tobytes()
    for ch in range(2):
        g = recs[0]["rec"][ch][:n[ch]]
        assert g["state"][-1] == 4 and np.count_nonzero(g["flags"] & gsdr.TRK_F_BIT_SYNC) == 1, ch


def test_pool_over_ring_equals_single_buffer():
    """Four E5a pilot channels (different PRNs, secondary codes, delays, Dopplers) in one
    handle, fed by uneven pushes through gsdr_trk_run_stream: the records of the single-buffer run."""
    fs, vl = 4.0e6, 4000
    spec = [(3, 1234.5, 1357), (8, -2210.0, 201), (21, 480.0, 3890), (40, 3050.0, 2222)]
    n = int(0.25 * fs)
    sats = [wb.satellite("5X", prn, fs, dop, start, cn0=46.0) for prn, dop, start in spec]
    iq = synth.e5a_iq(fs, n, sats, seed_offset=9)
    conf = _conf_sig(fs, gsdr.SIGNAL_GAL_5X, 4, 1)

    def started():
        t = gsdr.Tracking(conf)
        for ch, ((prn, dop, start), s) in enumerate(zip(spec, sats)):
            ci, cq = wb.primary_codes("5X", prn)
            t.start(ch, prn, cq, float(start), float(250 * round(dop / 250)), 0, 0, data_code=ci, secondary_code=s.sec_q)
        return t

    t = started()
    rec, cnt = t.run(iq, 0, 300)
    t.close()
    assert np.all(cnt >= 245)
    t = started()
    ring = gsdr.Stream(gsdr.ITEM_GR_COMPLEX, capacity_items=64 * vl, max_window_items=32 * vl)
    got = [[] for _ in spec]
    pushed = 0
    sizes = [3 * vl + 17, 7 * vl + 1, vl - 3, 12 * vl + 555, 5, 9 * vl]
    k = 0
    while pushed < n:
        m = min(sizes[k % len(sizes)], n - pushed)
        ring.push(iq[pushed:pushed + m], pushed)
        pushed += m
        k += 1
        r, c = t.run_stream_host(ring, 32)
        for ch in range(len(spec)):
            got[ch].append(r[ch][:c[ch]])
    ring.close()
    t.close()
    for ch in range(len(spec)):
        g = np.concatenate(got[ch])
        assert len(g) == cnt[ch], (ch, len(g), cnt[ch])
        assert g.tobytes() == rec[ch][:cnt[ch]].tobytes(), ch


def test_telemetry_fault_in_state_4():
    """gsdr_trk_force_loss_of_lock between two calls of state 4 on E5a pilot tracking: one
    loss-of-lock record, at the call where the replay with the same fault puts it."""
    c = wb.case("5X", 1)
    at = c.sync_call + 50
    t = gsdr.Tracking(c.conf())
    _start(t, 0, c)
    a, na = t.run(c.iq, 0, at)
    assert na[0] == at
    t.force_loss_of_lock(0)
    b, nb = t.run(c.iq, 0, 200)
    g = np.concatenate([a[0][:na[0]], b[0][:nb[0]]])
    assert len(g) == at + 1 and g["state"][at] == 4
    assert np.count_nonzero(g["flags"] & gsdr.TRK_F_LOSS_OF_LOCK) == 1 and g["flags"][at] & gsdr.TRK_F_LOSS_OF_LOCK
    assert t.channel(0)["state"] == 0
    t.close()
    o = c.restatement()[0].replay(g, force_before=[at])
    for f in ("sample_counter", "consumed", "state", "flags"):
        np.testing.assert_array_equal(g[f], o[f], err_msg=f)
    np.testing.assert_array_equal(g["prompt_i"], o["prompt_i"])
    np.testing.assert_array_equal(g["prompt_q"], o["prompt_q"])
    assert not np.any(c.restatement()[0].replay(g)["flags"] & gsdr.TRK_F_LOSS_OF_LOCK)


# ------------------------------------------------------------------ host mirror
EXE = os.path.join(ROOT, "gnss-sdr-new_amd", "build", "e5a_tracking_selftest")


def _secondary_table():
    """The user's E5a-Q secondary code file: 50 rows of 100 bits, MSB first, 13 bytes each."""
    bits = np.zeros((50, 13 * 8), np.uint8)
    for prn in range(1, 51):
        bits[prn - 1, :100] = [int(ch) for ch in wb.e5a_secondary(prn)]
    return np.packbits(bits, axis=1, bitorder="big").tobytes()


def _selftest(tmp_path, c, pooled, secondary_file):
    import json
    (tmp_path / "e5a_codes.bin").write_bytes(wb._e5a_table())
    (tmp_path / "iq.dat").write_bytes(np.ascontiguousarray(c.iq).tobytes())
    lines = ["GNSS-SDR.internal_fs_sps=%d" % int(c.fs), "Tracking_5X.implementation=Galileo_E5a_DLL_PLL_Tracking_MI355X",
             "Tracking_5X.item_type=gr_complex", "Tracking_5X.pll_bw_hz=15.0", "Tracking_5X.dll_bw_hz=1.0",
             "Tracking_5X.pull_in_time_s=0", "Tracking_5X.track_pilot=true", "Channels_5X.count=1",
             "Tracking_5X.mi355x_pool=%s" % ("true" if pooled else "false"),
             "Tracking_5X.e5a_code_table=%s" % (tmp_path / "e5a_codes.bin")]
    if secondary_file is not None:
        lines.append("Tracking_5X.e5a_secondary_code_table=%s" % secondary_file)
    (tmp_path / "trk.conf").write_text("\n".join(lines) + "\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("GSDR_GALILEO_E5A")}
    p = subprocess.run([EXE, str(tmp_path / "trk.conf"), str(tmp_path / "iq.dat"), "Tracking_5X", str(c.prn), repr(c.delay),
                        repr(c.dop)], capture_output=True, text=True, timeout=120, env=env)
    return p.returncode, json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("pooled", [False, True])
def test_host_mirror_emits_swapped_prompts(tmp_path, pooled):
    """Galileo_E5a_DLL_PLL_Tracking_MI355X built from a .conf that names both user tables:
    the Gnss_Synchro stream of the block equals the valid outputs of the engine driven
    directly (whose swapped prompts test_loop_parity_staged_window checks), 1 ms each."""
    c = wb.case("5X", 1)
    (tmp_path / "e5a_secondary.bin").write_bytes(_secondary_table())
    rc, r = _selftest(tmp_path, c, pooled, tmp_path / "e5a_secondary.bin")
    assert rc == 0 and r["built"] and r["pooled"] == pooled and r["vector_length"] == 4000, r.get("error")
    g = _run(c, 1400)
    v = g[(g["flags"] & gsdr.TRK_F_VALID_OUTPUT) != 0]
    outs = r["outputs"]
    n = min(len(outs), len(v))
    assert len(v) - 1 <= len(outs) <= len(v) + 1 and n >= 5, (len(outs), len(v))
    for o, e in zip(outs[:n], v[:n]):
        assert o[0] == int(e["sample_counter"]) and o[1] == e["prompt_i"] and o[2] == e["prompt_q"], (o, e)
        assert o[3] == 1 and o[4] == 1
    # the records the block saw carry the same pair
    for o, e in zip(outs[:n], r["records"][:n]):
        assert o[:3] == e[:3]


def test_host_mirror_refuses_missing_or_short_secondary_file(tmp_path):
    c = wb.case("5X", 1)
    rc, r = _selftest(tmp_path, c, False, None)
    assert rc == 1 and not r["built"] and "secondary" in r["error"]
    rc, r = _selftest(tmp_path, c, False, tmp_path / "absent.bin")
    assert rc == 1 and not r["built"] and "cannot be read" in r["error"]
    (tmp_path / "short.bin").write_bytes(_secondary_table()[:-1])
    rc, r = _selftest(tmp_path, c, False, tmp_path / "short.bin")
    assert rc == 1 and not r["built"] and "649 bytes" in r["error"]

"""The paired-code acquisition restatement (tests/pair_checks.py) on the CPU: the two-replica
identity the engine relies on, the committed Galileo capture, the dwell rule and the 8 ms
adapter's threshold.  No GPU."""
import os

import numpy as np
import pytest

import gsdr
import pair_checks as pc
from conftest import GOLDEN


@pytest.fixture(scope="module")
def gal_capture():
    return np.fromfile(os.path.join(GOLDEN, "Galileo_E1_ID_1_Fs_4Msps_8ms.dat"), np.complex64)


def _plain_rows(x, fs, dmax, dstep, replica):
    """Row maxima of the plain circular correlation with one replica, normalised as magt is."""
    N = len(x)
    f = np.conj(np.fft.fft(np.asarray(replica, np.complex128)))
    out = []
    for X in pc._spectra(x, fs, dmax, dstep):
        r = np.fft.ifft(X * f) * N
        out.append(np.max(r.real ** 2 + r.imag ** 2) / (float(N) * float(N)) ** 2)
    return np.array(out)


def test_two_replica_identity(gal_capture):
    """plus and minus, formed point by point from two inverse transforms, are the plain
    correlations with B - jC and B + jC."""
    c = pc.capture_case(gal_capture, pc.CCCWSR)
    x = gal_capture[:16000]
    mags, _, _ = pc.member_rows(x, c["fs"], c["dmax"], c["dstep"], pc.CCCWSR, c["first"], c["second"])
    B, C = c["first"].astype(np.complex128), c["second"].astype(np.complex128)
    peak = mags.max()
    for member, replica in ((0, B - 1j * C), (1, B + 1j * C)):
        plain = _plain_rows(x, c["fs"], c["dmax"], c["dstep"], replica)
        err = float(np.max(np.abs(plain - mags[:, member])) / peak)
        print("member %d: %.3g of the peak" % (member, err))
        assert err <= 1e-12


# (policy, slice of the capture) -> delay, Doppler, member, statistic, second row / first, member margin
CAPTURE = [
    (pc.CCCWSR, slice(0, 16000), 2920, -750, 0, 0.479, 0.92, 0.45),
    (pc.CCCWSR, slice(16000, 32000), 2920, -750, 0, 0.633, 0.94, 0.91),
    (pc.PCPS_8MS, slice(0, 32000), 2920, -500, 1, 0.079, 0.94, 0.38),
]


@pytest.mark.parametrize("policy,sl,delay,doppler,member,stat,second_row,member_margin", CAPTURE)
def test_capture(gal_capture, policy, sl, delay, doppler, member, stat, second_row, member_margin):
    c = pc.capture_case(gal_capture, policy)
    b = pc.block_record(gal_capture[sl], c["fs"], c["dmax"], c["dstep"], policy, c["first"], c["second"], c["spc"], 0)
    r, m = b["rec"], b["margins"]
    print(r, m)
    assert len(pc.doppler_rows(c["dmax"], c["dstep"])) == 81
    assert (r["acq_delay_samples"], r["doppler_hz"], r["member"]) == (delay, doppler, member)
    assert abs(r["test_statistic"] - stat) <= 1e-3
    assert abs((1.0 - m["row"]) - second_row) <= 1e-2
    assert abs(m["member"] - member_margin) <= 1e-2
    # the reference test's own bounds for this capture: 0.175 chip and 166 Hz of 2920 / -632
    assert abs(r["acq_delay_samples"] - 2920) / (4000000 / 1.023e6) <= 0.175
    assert abs(r["doppler_hz"] - (-632)) <= 166


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_margins(name):
    """Every record the GPU tests compare exactly is pinned: winner >= 1e-3 above its runner-up in
    row, member and index; the satellites meant to be found are found where they were put."""
    case = pc.pair_case(name)
    sats = pc.CASES[name]["sats"]
    for b in range(pc.NBLOCKS):
        for q, (prn, present, row, tau, member) in enumerate(sats):
            ref = case.reference(b, q)
            m = ref["margins"]
            assert min(m.values()) >= pc.MIN_MARGIN, (name, b, q, m)
            if present:
                r = ref["rec"]
                assert (r["doppler_index"], r["code_phase"] % case.spc, r["member"]) == (row, tau % case.spc, member), \
                    (name, b, q, r)


def _records(mags, ips, stamps):
    rec = np.zeros(len(mags), gsdr.ACQ_PAIR_RESULT_DTYPE)
    rec["mag"], rec["input_power"], rec["samplestamp"] = mags, ips, stamps
    rec["test_statistic"] = rec["mag"] / rec["input_power"]
    rec["acq_delay_samples"] = [10.0 + k for k in range(len(mags))]
    rec["doppler_hz"] = [250 * k for k in range(len(mags))]
    return rec


def _as_dicts(rec):
    return [dict(mag=float(r["mag"]), input_power=float(r["input_power"]), samplestamp=int(r["samplestamp"]),
                 acq_delay_samples=float(r["acq_delay_samples"]), doppler_hz=int(r["doppler_hz"])) for r in rec]


def test_pair_decide_carry_against_no_carry():
    # dwell 0 strong in a loud item, dwell 1 weak in a quiet one: only the carried d_mag passes
    rec = _records([0.8, 0.1], [4.0, 1.0], [0, 100])
    out, pos, n = gsdr.pair_decide(rec, 0.5, carry_mag=True)
    assert (pos, n) == (True, 2) and out["samplestamp"] == 0 and out["acq_delay_samples"] == 10.0
    assert out["mag"] == np.float32(0.8) and out["input_power"] == 1.0 and out["test_statistic"] == np.float32(0.8)
    out, pos, n = gsdr.pair_decide(rec, 0.5, carry_mag=False)
    assert (pos, n) == (False, 2) and out["samplestamp"] == 100 and out["test_statistic"] == np.float32(0.1)
    for carry in (True, False):
        ref, rpos, rn = pc.decide(_as_dicts(rec), 0.5, carry)
        got, pos, n = gsdr.pair_decide(rec, 0.5, carry)
        assert (pos, n, int(got["samplestamp"])) == (rpos, rn, ref["samplestamp"])
        assert abs(float(got["test_statistic"]) - ref["test_statistic"]) <= 1e-6


def test_pair_decide_tie_keeps_the_earlier_dwell():
    rec = _records([0.25, 0.25, 0.25], [1.0, 1.0, 1.0], [0, 100, 200])
    out, pos, n = gsdr.pair_decide(rec, 0.5, carry_mag=True)
    assert (pos, n) == (False, 3) and out["samplestamp"] == 0 and out["doppler_hz"] == 0
    out, pos, n = gsdr.pair_decide(rec, 0.5, carry_mag=False)
    assert (pos, n) == (False, 3) and out["samplestamp"] == 200


def test_pair_decide_stops_at_the_first_positive():
    rec = _records([0.1, 0.9, 0.95], [1.0, 1.0, 1.0], [0, 100, 200])
    for carry in (True, False):
        out, pos, n = gsdr.pair_decide(rec, 0.5, carry)
        assert (pos, n) == (True, 2) and out["samplestamp"] == 100
    # the statistic must exceed the threshold, not reach it
    out, pos, n = gsdr.pair_decide(_records([0.5], [1.0], [0]), 0.5, True)
    assert (pos, n) == (False, 1)


def test_pair_decide_negative_after_max_dwells():
    rec = _records([0.1, 0.2], [1.0, 1.0], [0, 100])
    out, pos, n = gsdr.pair_decide(rec, 0.5, carry_mag=True)
    assert (pos, n) == (False, 2) and out["samplestamp"] == 100 and out["mag"] == np.float32(0.2)


def test_pair_result_layout_matches_c_compiler(tmp_path):
    """ACQ_PAIR_RESULT_DTYPE against sizeof / offsetof of gsdr_acq_pair_result, and the constants."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dt = gsdr.ACQ_PAIR_RESULT_DTYPE
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsdr.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(gsdr_acq_pair_result));',
             'printf("AS_IS %d\\nSUM_DIFF_J %d\\n", GSDR_ACQ_PAIR_AS_IS, GSDR_ACQ_PAIR_SUM_DIFF_J);']
    lines += ['printf("%s %%zu\\n", offsetof(gsdr_acq_pair_result, %s));' % (f, f) for f in dt.names]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0;}"]))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == dt.itemsize
    assert (int(got["AS_IS"]), int(got["SUM_DIFF_J"])) == (gsdr.PAIR_AS_IS, gsdr.PAIR_SUM_DIFF_J)
    for f in dt.names:
        assert int(got[f]) == dt.fields[f][1], f


def test_null_arguments_are_rejected_without_a_device():
    L = gsdr.load()
    assert L.gsdr_acq_set_code_pairs(None, 0, None, None, None, 1) == gsdr.GSDR_E_ARG
    assert b"null" in L.gsdr_last_error()
    assert L.gsdr_acq_run_pairs(None, None, 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_run_pairs_stream(None, None, 0, 1, 0, None) == gsdr.GSDR_E_ARG
    assert L.gsdr_acq_dump_pair_rows(None, None, None) == gsdr.GSDR_E_ARG


def test_threshold_8ms_and_key_rounding():
    for pfa, vl, dmax, dstep in ((0.001, 32000, 10000, 250), (0.1, 32000, 500, 250), (1e-5, 16000, 5000, 125)):
        ncells = vl * len(range(-dmax, dmax + 1, dstep))
        want = -np.log1p(-(1.0 - float(np.float32(pfa))) ** (1.0 / ncells)) / vl
        assert abs(pc.threshold_8ms(pfa, vl, dmax, dstep) - want) <= 1e-7 * want
    assert [pc.sampled_ms_key(v) for v in (4, 5, 7, 8, 9, 11, 12)] == [4, 4, 4, 8, 8, 8, 12]

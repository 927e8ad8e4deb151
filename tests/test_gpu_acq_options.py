"""Documented kernel options that only the profile scripts ran, against the fp64 oracle
(acq_checks.check_size: forward spectra, the grid of a visible PRN, the result records)
on the small grid of test_gpu_acq_sizes (8 Doppler rows, 3 visible PRNs of 4 slots).
Each option is set in the environment before the handle is created and read back
through gsdr_acq_get_split:

  GSDR_ACQ_PPW=2  25000: two PRNs per 1024-lane workgroup (split id 25); a launch with
                  an odd active PRN count runs one PRN per workgroup on the same plan
  GSDR_ACQ_QPW=1  100000 = 4 x 25000: one sub-transform per workgroup (split id 4; the
                  default, two per workgroup, is id 24)
  GSDR_ACQ_SPLIT=0  100000 on the packed four-step's general kernels (no split)
  GSDR_ACQ_SPLIT_ARG=0  25000: the split path's selected rows recomputed on the packed
                  four-step plan instead of on the split plan

Every switch is read when the handle is created and kept in it, GSDR_ACQ_SPLIT_ARG
included, so handles created under different settings coexist in one process.
"""
import pytest

import gsdr
from acq_checks import check_records, check_size, make_acq, size_case

pytestmark = pytest.mark.gpu

PFAS = [0.01, 0.0]


def _ppw1_records(monkeypatch, case, pfa, nprn):
    monkeypatch.setenv("GSDR_ACQ_PPW", "1")
    ref = make_acq(case, pfa, nprn=nprn)
    assert ref.plan["split"] == 1
    res = ref.run(case.x)[0]
    check_records(res, ref, case, pfa)
    ref.close()
    return res


@pytest.mark.parametrize("nprn", [4, 3])
@pytest.mark.parametrize("pfa", PFAS)
def test_ppw2_25000(monkeypatch, pfa, nprn):
    """Two PRNs per workgroup with 4 active PRNs (the paired kernel) and with 3 (the
    odd-count fallback): the oracle checks, and records byte-identical to the
    one-PRN-per-workgroup run of the same input (itself checked against the oracle, so
    a difference names the side that is off)."""
    case = size_case(25000)
    ref = _ppw1_records(monkeypatch, case, pfa, nprn)
    monkeypatch.setenv("GSDR_ACQ_PPW", "2")
    acq = make_acq(case, pfa, nprn=nprn)
    plan = acq.plan
    assert plan["split"] == 25 and plan["variant"] == 27, plan
    res = check_size(acq, case, pfa, "ppw2_%dprn" % nprn)
    assert len(res) == nprn
    assert res.tobytes() == ref.tobytes()
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_ppw2_active_count_changes(monkeypatch, pfa):
    """One PPW = 2 handle from 4 active PRNs to 3 (odd: the fallback kernel) and back to 4."""
    case = size_case(25000)
    ref4 = _ppw1_records(monkeypatch, case, pfa, 4)
    ref3 = _ppw1_records(monkeypatch, case, pfa, 3)
    monkeypatch.setenv("GSDR_ACQ_PPW", "2")
    acq = make_acq(case, pfa)
    assert acq.plan["split"] == 25
    for nprn, ref in ((4, ref4), (3, ref3), (4, ref4)):
        acq.set_active_prns(nprn)
        res = acq.run(case.x)[0]
        assert len(res) == nprn
        check_records(res, acq, case, pfa)
        assert res.tobytes() == ref.tobytes(), nprn
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_split_arg_off_25000(monkeypatch, pfa):
    """GSDR_ACQ_SPLIT_ARG=0: the grid maximum's row recomputed on the packed four-step
    (variant 27) for the first-maximum index, peak and CFAR power / second peak.  A
    handle created afterwards without the switch, in the same process, is back on the
    split plan's own pass: both pass the oracle checks and agree on every decision,
    but their peaks are not bit-identical -- 25000 = 25 x (10 x 10 x 10) and 5 x (25 x
    20 x 10) round differently (the oracle comparison in test_gpu_acq_sizes puts either
    engine ~2e-7 from fp64, not at it), which is how the test tells the two paths apart."""
    case = size_case(25000)
    monkeypatch.setenv("GSDR_ACQ_PPW", "1")
    monkeypatch.setenv("GSDR_ACQ_SPLIT_ARG", "0")
    off = make_acq(case, pfa)
    assert off.plan["split"] == 1 and off.plan["variant"] == 27, off.plan
    res_off = check_size(off, case, pfa, "split_arg0")
    monkeypatch.delenv("GSDR_ACQ_SPLIT_ARG")
    dflt = make_acq(case, pfa)
    assert dflt.plan["split"] == 1 and dflt.plan["variant"] == 27, dflt.plan
    res_dflt = check_size(dflt, case, pfa, "split_arg_default")
    for f in ("prn", "doppler_index", "code_phase", "doppler_hz", "positive"):
        assert (res_off[f][:case.nvis] == res_dflt[f][:case.nvis]).all(), f
    print("split_arg peaks off/default:", res_off["peak"], res_dflt["peak"])
    assert res_off["peak"].tobytes() != res_dflt["peak"].tobytes()
    # the first handle is still on its own path
    assert off.run(case.x)[0].tobytes() == res_off.tobytes()
    off.close()
    dflt.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_qpw1_100000(monkeypatch, pfa):
    """100000 = 4 x 25000 with one sub-transform per 512-lane workgroup."""
    monkeypatch.setenv("GSDR_ACQ_QPW", "1")
    case = size_case(100000)
    acq = make_acq(case, pfa)
    plan = acq.plan
    assert plan["split"] == 4 and plan["variant"] == 26, plan
    check_size(acq, case, pfa, "qpw1")
    acq.close()


@pytest.mark.parametrize("pfa", PFAS)
def test_split_off_100000(monkeypatch, pfa):
    """The third path at 100000 (bit transition off): GSDR_ACQ_SPLIT=0, the packed
    four-step's own correlate; the default (QPW = 2, split id 24) is what the C5
    Galileo tests run."""
    monkeypatch.setenv("GSDR_ACQ_QPW", "1")
    monkeypatch.setenv("GSDR_ACQ_SPLIT", "0")
    case = size_case(100000)
    acq = make_acq(case, pfa)
    plan = acq.plan
    assert plan["split"] == 0 and plan["variant"] == 26, plan
    check_size(acq, case, pfa, "split_off")
    acq.close()

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

GSDR_ACQ_SPLIT_ARG is read once per process into a static and cannot be toggled here.
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

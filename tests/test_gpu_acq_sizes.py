"""The acquisition engine at the FFT sizes no configuration of the benchmark uses,
against an fp64 oracle, through the C ABI.

Any N = 2^a 3^b 5^c is accepted: up to 20352 points on an LDS plan the host planner
picks at run time (fft_plan.h make_plan, kernels RuntimePlan<256 | 512 | 1024> built
from fft_lds.h stage<R, NT, FIRST, LAST>), beyond that -- or where no thread budget
admits an LDS plan -- as the generic four-step R x N2 (FourStepPlan<256 | 1024>,
variants 20 / 22).  The lists below reach every radix of the runtime path in every
stage position the planner can give it, plans of 3 to 8 stages, the three workgroup
sizes and the register radices R = 10, 12, 16, 20, 25 of the four-step.  R = 8 is in
choose_variant's list but unreachable: it is tried last, and a size divisible by 8 but
by none of 25, 20, 16, 12, 10 has no factor 3 or 5 and only 2^3, i.e. N = 8; it is not
forced here.

Per size: one block of 1 ms GPS C/A at fs = 1000 N, 8 Doppler rows (+-1000 Hz, 250 Hz),
4 PRN slots (3 visible at 50 dB-Hz, 1 absent), gr_complex input, and the three checks of
acq_checks.check_size: forward spectra within 2e-6 (norm-relative, every Doppler row) of
numpy's fp64 FFT, the |R|^2 grid of a visible PRN within 1e-5 of its maximum of the
oracle grid, and the result records of both statistics (pfa = 0.01 CFAR, pfa = 0 peak
ratio) on the oracle's cells.  test_plan_coverage pins what the lists reach, so a planner
change cannot silently empty the sweep.

Measured on an MI355X when the sweep was added (spectrum error / grid error; bounds 2e-6
and 1e-5), N [plan]:
  256 threads:  1125 [25,5,3,3] 1.5e-7/1.8e-7, 1215 [5,3x5] 1.6e-7/4.8e-8, 1944 [12,6,3,3,3]
                1.4e-7/2.9e-7, 2048 [16,16,8] 1.5e-7/2.6e-7, 2430 [10,3x5] 1.4e-7/1.6e-7,
                3000 [25,20,6] 1.6e-7/2.1e-7, 4096 [16,16,16] 1.3e-7/2.4e-7, 4374 [6,3x6]
                2.1e-7/4.0e-7, 5000 [25,20,10] 1.5e-7/2.8e-7
  512 threads:  6000 [25,20,12] 1.4e-7/3.3e-7, 6561 [3x8] 1.7e-7/3.2e-7, 9000 [25,20,6,3]
                1.8e-7/1.8e-7, 10000 [25,20,20] 1.7e-7/2.3e-7
  1024 threads: 12000 [25,20,12,2] 1.6e-7/2.1e-7, 12500 [25,25,20] 2.0e-7/4.3e-7, 15625
                [25,25,25] 1.7e-7/3.7e-7, 16384 [16,16,16,4] 1.6e-7/2.6e-7, 20000 [20,20,10,5]
                1.9e-7/3.7e-7
  four-step, 256 threads (R x [N2 plan]): 19200 25x[16,16,3] 1.6e-7/1.9e-7, 20480 20x[16,16,4]
                1.8e-7/2.4e-7, 21870 10x[3x7] 1.7e-7/4.0e-7, 26244 12x[3x7] 2.0e-7/3.8e-7,
                32768 16x[16,16,8] 1.6e-7/2.5e-7, 40000 25x[25,16,4] 1.7e-7/3.0e-7, 80000
                25x[25,16,8] 1.7e-7/1.9e-7; GSDR_ACQ_FOUR_GENERIC=1: 25000 25x[25,20,2]
                1.9e-7/3.6e-7, 32000 25x[20,16,4] 1.4e-7/2.5e-7
  four-step, 1024 threads: 73728 16x[16,16,6,3] 1.9e-7/5.7e-7, 128000 25x[20,16,16]
                1.7e-7/1.9e-7
Sensitivity, from a library altered on purpose: one twiddle of the later radix-12 stages
off by one table stride gives 2.5e-4 / 1.0e-4 at 6000 and 3.5e-4 / 1.0e-4 at 12000, one
wrong inter-step twiddle of the R = 10 columns 0.32 / 0.22 at 21870; no other size moves.
"""
import numpy as np
import pytest

import gsdr
from acq_checks import check_size, make_acq, size_case

pytestmark = pytest.mark.gpu

# N -> (workgroup threads, plan) of the runtime-planned LDS FFT
LDS_PLANS = {
    1125: (256, [25, 5, 3, 3]),
    1215: (256, [5, 3, 3, 3, 3, 3]),
    1944: (256, [12, 6, 3, 3, 3]),
    2048: (256, [16, 16, 8]),
    2430: (256, [10, 3, 3, 3, 3, 3]),
    3000: (256, [25, 20, 6]),
    4096: (256, [16, 16, 16]),
    4374: (256, [6, 3, 3, 3, 3, 3, 3]),
    5000: (256, [25, 20, 10]),
    6000: (512, [25, 20, 12]),
    6561: (512, [3, 3, 3, 3, 3, 3, 3, 3]),
    9000: (512, [25, 20, 6, 3]),
    10000: (512, [25, 20, 20]),
    12000: (1024, [25, 20, 12, 2]),
    12500: (1024, [25, 25, 20]),
    15625: (1024, [25, 25, 25]),
    16384: (1024, [16, 16, 16, 4]),
    20000: (1024, [20, 20, 10, 5]),
}
# N -> (R, N2, threads) of the generic four-step; 19200 is below the LDS limit, but no
# thread budget admits an LDS plan for it
FOUR_PLANS = {
    19200: (25, 768, 256),
    20480: (20, 1024, 256),
    21870: (10, 2187, 256),
    26244: (12, 2187, 256),
    32768: (16, 2048, 256),
    40000: (25, 1600, 256),
    80000: (25, 3200, 256),
    73728: (16, 4608, 1024),
    128000: (25, 5120, 1024),
}
# sizes of the packed four-step kept on the generic one by GSDR_ACQ_FOUR_GENERIC=1
GENERIC_AT_PACKED = [25000, 32000]
PFAS = [0.01, 0.0]


def _positions(radix):
    """(radix, position) pairs of a plan: first, middle(s), last."""
    n = len(radix)
    return {(r, "first" if i == 0 else ("last" if i == n - 1 else "middle")) for i, r in enumerate(radix)}


@pytest.mark.parametrize("N,pfa", [(N, pfa) for N in LDS_PLANS for pfa in PFAS])
def test_lds_runtime_sizes(N, pfa):
    """Runtime-planned LDS sizes (variants 10-12), 6000 and 10000 of the older tests included."""
    case = size_case(N)
    acq = make_acq(case, pfa)
    plan = acq.plan
    assert plan["variant"] in (10, 11, 12) and plan["r1"] == 0 and plan["split"] == 0
    assert int(np.prod(plan["radix"])) == N
    check_size(acq, case, pfa, "lds_runtime")
    acq.close()


@pytest.mark.parametrize("N,pfa", [(N, pfa) for N in FOUR_PLANS for pfa in PFAS])
def test_generic_four_step_sizes(N, pfa):
    """Generic four-step sizes (variants 20 / 22): Galileo E1 / GPS at rates other than
    the benchmark's, and 19200, which no LDS thread budget admits."""
    case = size_case(N)
    acq = make_acq(case, pfa)
    plan = acq.plan
    assert plan["variant"] in (20, 22) and plan["split"] == 0
    assert plan["r1"] * int(np.prod(plan["radix"])) == N
    check_size(acq, case, pfa, "four_generic")
    acq.close()


@pytest.mark.parametrize("split", ["1", "0"])
@pytest.mark.parametrize("N,pfa", [(N, pfa) for N in GENERIC_AT_PACKED for pfa in PFAS])
def test_generic_four_step_at_packed_sizes(monkeypatch, N, pfa, split):
    """GSDR_ACQ_FOUR_GENERIC=1 at 25000 / 32000: forward, dumps and (GSDR_ACQ_SPLIT=0) the
    correlate on the generic four-step; with the split correlate left on, its row maxima
    over the generic forward spectra."""
    monkeypatch.setenv("GSDR_ACQ_FOUR_GENERIC", "1")
    monkeypatch.setenv("GSDR_ACQ_SPLIT", split)
    case = size_case(N)
    acq = make_acq(case, pfa)
    plan = acq.plan
    assert plan["variant"] == 20 and plan["nstages"] >= 2, plan
    assert (plan["split"] != 0) == (split == "1"), plan
    check_size(acq, case, pfa, "four_generic_at_packed")
    acq.close()


def test_plan_coverage(monkeypatch):
    """What the size lists reach, read back through gsdr_acq_get_plan (handles only, no
    launch beyond their set-up): every radix of the runtime path in every position of the
    tables above, the three workgroup sizes on variants 10-12, stage counts 3 to 8, the
    four-step's register radices 10 / 12 / 16 / 20 / 25 on variant 20 and variant 22 twice;
    and the sizes neither path takes are refused."""
    seen_pos, seen_nt, seen_stages, seen_r20, n22 = set(), set(), set(), set(), 0
    for N, (nt, radix) in LDS_PLANS.items():
        acq = gsdr.Acquisition(1000 * N, N, 1000, 250, pfa=0.01, max_prns=1)
        p = acq.plan
        acq.close()
        assert p["variant"] == {256: 10, 512: 11, 1024: 12}[p["nthreads"]], (N, p)
        assert (p["nthreads"], p["radix"]) == (nt, radix) and p["nstages"] == len(radix) and p["r1"] == 0, (N, p)
        seen_pos |= _positions(p["radix"])
        seen_nt.add(p["nthreads"])
        seen_stages.add(p["nstages"])
    want_pos = set().union(*(_positions(r) for _, r in LDS_PLANS.values()))
    # the tables' pairs: 8 first, 8 middle and 11 last positions over the 11 radices
    assert len(want_pos) == 27 and seen_pos >= want_pos
    assert {r for r, _ in seen_pos} == {2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 25}
    assert {r for r, pos in seen_pos if pos != "last"}.isdisjoint({2, 4, 8})
    assert seen_nt == {256, 512, 1024}
    assert seen_stages >= {3, 4, 5, 6, 7, 8}
    for N, (r1, n2, nt) in FOUR_PLANS.items():
        acq = gsdr.Acquisition(1000 * N, N, 1000, 250, pfa=0.01, max_prns=1)
        p = acq.plan
        acq.close()
        assert p["variant"] == {256: 20, 1024: 22}[p["nthreads"]], (N, p)
        assert (p["r1"], int(np.prod(p["radix"])), p["nthreads"]) == (r1, n2, nt) and p["nstages"] >= 2, (N, p)
        if p["variant"] == 20:
            seen_r20.add(p["r1"])
        else:
            n22 += 1
    assert seen_r20 == {10, 12, 16, 20, 25}
    assert n22 >= 2
    # the packed four-step reports its compile-time sub-plan as 0 stages
    acq = gsdr.Acquisition(25000000, 25000, 1000, 250, pfa=0.01, max_prns=1)
    p = acq.plan
    acq.close()
    assert (p["variant"], p["r1"], p["nstages"], p["radix"], p["split"]) == (27, 5, 0, [], 1), p
    monkeypatch.setenv("GSDR_ACQ_FOUR_GENERIC", "1")
    for N in GENERIC_AT_PACKED:
        acq = gsdr.Acquisition(1000 * N, N, 1000, 250, pfa=0.01, max_prns=1)
        p = acq.plan
        acq.close()
        assert p["variant"] == 20 and p["r1"] == 25 and p["r1"] * int(np.prod(p["radix"])) == N, (N, p)
    for N in (19683, 6625):  # 3^9: nine stages and no register radix divides it; 5^3 * 53
        with pytest.raises(gsdr.GsdrError) as e:
            gsdr.Acquisition(1000 * N, N, 1000, 250)
        assert e.value.code == gsdr.GSDR_E_UNSUPPORTED

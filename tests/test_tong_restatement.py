"""The float64 restatement of the Tong block (tong_checks.py) against the pure-Python pieces of the
package and against the reference's own test vector.  No GPU."""
import math
import os

import numpy as np
import pytest

import gsdr
import tong_checks as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T, INIT, TMAX, MAXD = 1.0, 2, 4, 8

# statistic sequences (the accumulated grid's maximum per dwell) and the path they must take
SEQUENCES = {
    # straight up: 2 -> 3 -> 4, positive on dwell 2; what follows is past the end
    "up": ([1.5, 3.0, 9.9, 0.0], [(1, 3, 0), (2, 4, 1), (2, 4, 3), (2, 4, 3)]),
    # straight down: 2 -> 1 -> 0, negative on dwell 2
    "down": ([0.5, 1.0, 9.9], [(1, 1, 0), (2, 0, 2), (2, 0, 3)]),
    # up, down, up, up: positive on dwell 4 (2.0 is not above 2 T: strict '>')
    "up-down-up": ([1.5, 2.0, 3.5, 4.5], [(1, 3, 0), (2, 2, 0), (3, 3, 0), (4, 4, 1)]),
    # an oscillation that tong_max_dwells ends with the count at 2
    "cut": ([1.5, 1.5, 1.5, 4.5, 5.5, 5.5, 5.5, 8.5, 0.0],
            [(1, 3, 0), (2, 2, 0), (3, 1, 0), (4, 2, 0), (5, 3, 0), (6, 2, 0), (7, 1, 0), (8, 2, 2), (8, 2, 3)]),
    # the count reaches tong_max_val on the very dwell that equals tong_max_dwells: negative
    "overridden": ([0.5, 2.5, 3.5, 3.5, 3.5, 6.5, 7.5, 8.5],
                   [(1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 2, 0), (5, 1, 0), (6, 2, 0), (7, 3, 0), (8, 4, 2)]),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_tong_decide_follows_the_block(name):
    stats, path = SEQUENCES[name]
    ref = tc.block_decisions(stats, T, INIT, TMAX, MAXD)
    assert ref == path
    assert [c[:3] for c in tc.counter(stats, T, INIT, TMAX, MAXD)] == path
    assert gsdr.tong_decide(stats, T, INIT, TMAX, MAXD) == path


def test_tong_decide_defaults_of_the_adapters():
    """tong_init_val 1, tong_max_val 2, tong_max_dwells 3: one dwell decides."""
    assert gsdr.tong_decide([2.0, 0.0], 1.0, 1, 2, 3) == [(1, 2, 1), (1, 2, 3)] == tc.block_decisions([2.0, 0.0], 1.0, 1, 2, 3)
    assert gsdr.tong_decide([0.5], 1.0, 1, 2, 3) == [(1, 0, 2)] == tc.block_decisions([0.5], 1.0, 1, 2, 3)


def test_tong_decide_rejects_counters_the_reference_cannot_run():
    for init, tmax, maxd in ((0, 2, 3), (2, 2, 3), (3, 2, 3), (1, 2, 0)):
        with pytest.raises(AssertionError):
            gsdr.tong_decide([1.0], 1.0, init, tmax, maxd)


@pytest.mark.parametrize("pfa,n,bins", [(0.001, 4000, 81), (1e-6, 16000, 41), (0.1, 2000, 9)])
def test_tong_threshold(pfa, n, bins):
    """calculate_threshold of both adapters: quantile(exponential(lambda = n), (1 - pfa)^(1 / (n bins)))."""
    val = math.pow(1.0 - float(np.float32(pfa)), 1.0 / float(n * bins))
    want = float(np.float32(-math.log1p(-val) / float(n)))
    got = gsdr.tong_threshold(pfa, n, bins)
    assert got == want == tc.threshold(pfa, n, bins)
    # the quantile's defining property: P(X <= t) = val for the exponential with that rate
    assert abs(1.0 - math.exp(-float(n) * got) - val) < 1e-7 * val
    assert got > 0.0


def test_cases_meet_their_conditions():
    """Every winner at least MIN_MARGIN above its runner-up and every statistic at least MIN_DECISION
    from threshold * dwell, on the restatement alone, for every item type the GPU tests use; and the
    paths the cases are built for."""
    for name in tc.CASES:
        c = tc.tong_case(name)
        for it in (0, 1, 2):
            for stream in (0, 1):
                for slot in (0, 1, 2):
                    tc.assert_margins(c.reference(stream, slot, 0, tc.NITEMS, it)[0])
        path = lambda s, q: [(r["dwell_count"], r["tong_count"], r["state"]) for r in c.reference(s, q)[0]]
        assert path(0, 0)[:3] == [(1, 3, 0), (2, 4, 1), (2, 4, 3)]            # positive after two dwells
        assert path(0, 1)[:3] == [(1, 1, 0), (2, 0, 2), (2, 0, 3)]            # negative after two, absent PRN
        assert path(0, 2) == SEQUENCES["cut"][1][:8]                          # cut by tong_max_dwells
        assert path(1, 0) == SEQUENCES["overridden"][1] == path(1, 2)         # the overridden positive, twice
        assert path(1, 1)[:5] == SEQUENCES["up-down-up"][1] + [(4, 4, 3)]     # up, down, up
        last = c.reference(0, 2)[0][0]
        assert (last["doppler_index"], last["indext"]) == (tc.D - 1, c.n - 1)  # the last row, delay N - 1


def test_capture():
    """The reference's own test vector: Doppler 1680 Hz, delay 524 samples, on both 1 ms items."""
    k = tc.capture_case()
    x = np.fromfile(os.path.join(GOLDEN, "GPS_L1_CA_ID_1_Fs_4Msps_2ms.dat"), np.complex64)
    assert len(x) == 2 * k["n"]
    thr = tc.threshold(0.001, k["n"], 81)
    recs, grids = tc.sequence_records([x[:k["n"]], x[k["n"]:]], k["fs"], k["dmax"], k["dstep"], k["code"], k["spc"], thr,
                                      1, 2, 3)
    assert grids[0].shape == (81, 4000)
    for g in grids:  # after item 1 and after both: the row nearest 1680 Hz, delay 524
        row, idx, _, margin = tc.winner(g)
        assert (row, idx) == (47, 524) and margin > 50 * tc.MIN_MARGIN
    assert recs[0]["doppler_hz"] == 1750 and recs[0]["acq_delay_samples"] == 524.0
    # the adapters' default counter decides on the first item
    assert recs[0]["state"] == tc.POSITIVE and recs[1]["state"] == tc.PAST_END


def test_speculation_is_exact():
    """Records of a sequence that ends at item k do not depend on what follows in the same call: item j's
    grid is a function of items <= j alone."""
    c = tc.tong_case("t2000")
    x = c.items(0)[1]
    st = c.streams[0]
    args = (c.fs, c.dmax, c.dstep, st["codes"][0], c.spc, tc.THRESHOLD, tc.INIT, tc.TMAX, tc.MAX_DWELLS)
    full, gfull = tc.sequence_records([x[k] for k in range(4)], *args)
    other, gother = tc.sequence_records([x[0], x[1], x[7], 3.0 * x[5]], *args)
    alone, galone = tc.sequence_records([x[0], x[1]], *args)
    assert full[1]["state"] == tc.POSITIVE
    assert full[:2] == other[:2] == alone
    assert all(np.array_equal(gfull[k], gother[k]) and np.array_equal(gfull[k], galone[k]) for k in range(2))
    # and past the end only the item's own properties remain
    for a, b in zip(full[2:], other[2:]):
        assert a["state"] == b["state"] == tc.PAST_END
        assert (a["dwell_count"], a["tong_count"], a["mag"], a["indext"]) == (2, 4, 0.0, 0) == \
            (b["dwell_count"], b["tong_count"], b["mag"], b["indext"])


def test_block_state_machine():
    """States 0-3 with their consume counts, the sample counter (the stamp is the item's end) and events."""
    c = tc.tong_case("t2000")
    st = c.streams[0]
    x = st["x"].reshape(-1).astype(np.complex128)
    b = tc.RefBlock(c.fs, c.n, c.spc, c.dmax, c.dstep, tc.THRESHOLD, tc.INIT, tc.TMAX, tc.MAX_DWELLS,
                    code=st["codes"][0], monitor=True)
    first, second = tc.run_attempts(b, x, 2, per_call=1)
    # state 0 consumes what is offered (item 0) and arms; item 1 (present) and item 2 (absent, but 3 T
    # stays above 2 T) go one per call; state 2 publishes and consumes item 3
    calls = first["calls"]
    assert [(q["state"], q["consumed"], q["event"]) for q in calls] == [(0, 1, 0), (1, 1, 0), (1, 1, 0), (2, 1, 1)]
    assert [(q["dwell_count"], q["tong_count"]) for q in calls[1:3]] == [(1, 3), (2, 4)]
    assert calls[2]["acq_samplestamp_samples"] == 3 * c.n and calls[2]["acq_doppler_step"] == c.dstep
    assert calls[3]["monitor"]["acq_delay_samples"] == float(c.n // 3 + 1)
    assert calls[3]["monitor"]["acq_doppler_hz"] == float(c.rows[2])
    assert first["sample_counter"] == 4 * c.n and first["end_state"] == 0
    # the second attempt starts from zero on items 5 and 6, where the satellite is absent: negative
    calls = second["calls"]
    assert [(q["state"], q["consumed"], q["event"]) for q in calls] == [(0, 1, 0), (1, 1, 0), (1, 1, 0), (3, 1, 2)]
    assert [(q["dwell_count"], q["tong_count"]) for q in calls[1:3]] == [(1, 1), (2, 0)]
    assert calls[3]["monitor"] is None and second["sample_counter"] == 8 * c.n

"""CPU: tests/norm_model.py, the restatement of the normalisation contract (rcorrector_amd/csrc/rc_norm.h), on hand-worked cases
-- the draw against splitmix64's published outputs -- and its keep rate against the binomial: 100 000 units of D = 4 * target keep
25 000 +- 685, five standard deviations of sqrt(100 000 * 1/4 * 3/4) = 137, for three seeds."""
import pytest

import norm_model as nm


def test_the_draw_is_the_upper_half_of_splitmix64():
    # the generator's well-known streams: state = seed, each output adds the golden gamma and finalises
    assert [nm.draw(0, i) for i in range(3)] == [0xE220A8397B1DCDAF >> 32, 0x6E789E6AA1B965F4 >> 32, 0x06C45D188009454F >> 32]
    want = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    assert [nm.draw(1234567, i) for i in range(5)] == [w >> 32 for w in want]
    # 64-bit wrap: index 2^64 - 1 gives z = seed; the seed and the index are not interchangeable
    assert nm.draw(0, nm.M64) == 0 and nm.draw(5, (1 << 32) + 7) != nm.draw((1 << 32) + 7, 5)
    assert nm.draw(0, 1 << 32) != nm.draw(0, 0)


def test_unit_depth_by_hand():
    assert nm.unit_depth([(10, 1, 7, 9)]) == 7
    assert nm.unit_depth([(0, 0, 0, 0)]) is None and nm.unit_depth([(0, 5, 5, 5), (0, 9, 9, 9)]) is None
    assert nm.unit_depth([(3, 1, 7, 9), (0, 0, 99, 0)]) == 7 and nm.unit_depth([(0, 0, 99, 0), (1, 4, 4, 4)]) == 4
    assert nm.unit_depth([(3, 1, 7, 9), (3, 1, 8, 9)]) == 8          # (7 + 8 + 1) >> 1: halves round up
    assert nm.unit_depth([(3, 1, 7, 9), (3, 1, 9, 9)]) == 8 and nm.unit_depth([(1, 0, 0, 0), (1, 0, 0, 0)]) == 0
    assert nm.unit_depth([(1, 0, 0, 0), (1, 1, 1, 1)]) == 1
    top = (1 << 31) - 1
    assert nm.unit_depth([(1, 0, top, top), (1, 0, top, top)]) == top    # m1 + m2 + 1 = 2^32 - 1: no overflow
    assert nm.unit_depth([(1, 0, top, top), (1, 0, top - 1, top)]) == top


def test_outcome_by_hand():
    R0, RMAX = 0, (1 << 32) - 1
    assert nm.outcome(None, R0, 10, 0) == nm.NOVALID
    assert nm.outcome(4, R0, 10, 5) == nm.LOW and nm.outcome(5, R0, 10, 5) == nm.KEPT
    assert nm.outcome(3, R0, 2, 5) == nm.LOW                       # low wins over the draw and over D <= target
    assert nm.outcome(0, RMAX, 10, 0) == nm.KEPT and nm.outcome(10, RMAX, 10, 0) == nm.KEPT
    assert nm.outcome(11, RMAX, 10, 0) == nm.OVER and nm.outcome(11, R0, 10, 0) == nm.KEPT
    # D = 2 * target: kept exactly for r < 2^31
    assert nm.outcome(20, (1 << 31) - 1, 10, 0) == nm.KEPT and nm.outcome(20, 1 << 31, 10, 0) == nm.OVER
    # D = 3, target = 1: r * 3 < 2^32, so r <= 1431655765
    assert nm.outcome(3, 1431655765, 1, 0) == nm.KEPT and nm.outcome(3, 1431655766, 1, 0) == nm.OVER
    top = (1 << 31) - 1
    assert nm.outcome(top, RMAX, top, 0) == nm.KEPT and nm.outcome(top, 1, 1, 0) == nm.KEPT and nm.outcome(top, 3, 1, 0) == nm.OVER
    assert nm.outcome(top, 2, 1, 0) == nm.KEPT                     # 2 * (2^31 - 1) < 2^32


def test_select_tallies_by_hand():
    rows = [(5, 1, 2, 3), (0, 0, 0, 0), (5, 1, 8, 9), (5, 1, 300, 400), (0, 0, 0, 0), (0, 0, 0, 0), (4, 1, 40, 50), (4, 1, 41, 50)]
    # mode 2: units (2, -) -> D 2; (8, 300) -> 154; novalid; (40, 41) -> 41.  target 1000: nothing is over
    keep, tally, depths = nm.select(rows, 4, 2, 0, 1000, 3, 9, 100)
    assert depths == [2, 154, None, 41] and keep == [nm.LOW, nm.KEPT, nm.NOVALID, nm.KEPT]
    before, after = tally[4:4 + 101], tally[4 + 101:]
    assert tally[:4] == [0, 2, 1, 1] and len(tally) == 4 + 2 * 101
    assert {i: n for i, n in enumerate(before) if n} == {2: 1, 41: 1, 100: 1} and {i: n for i, n in enumerate(after) if n} == {41: 1, 100: 1}
    # mode 1: read u with read 4 + u -> (2, -), (-, -), (8, 40), (300, 41); mode 0: every read alone; a second call adds up
    assert nm.select(rows, 4, 1, 0, 1000, 0, 9, 100)[2] == [2, None, 24, 171]
    keep0, tally0, depths0 = nm.select(rows, 8, 0, 0, 1000, 0, 9, 100, tally=tally)
    assert depths0 == [2, None, 8, 300, None, None, 40, 41] and tally0[:4] == [0, 7, 1, 4] and tally[:4] == [0, 2, 1, 1]
    # the draw is keyed by unit_base + u: a batch cut in two decides as the whole does
    deep = [(9, 1, 4000, 5000)] * 64
    whole = nm.select(deep, 64, 0, (1 << 32) + 5, 1000, 0, 77, 10)[0]
    assert whole == nm.select(deep[:20], 20, 0, (1 << 32) + 5, 1000, 0, 77, 10)[0] + nm.select(deep[20:], 44, 0, (1 << 32) + 25, 1000, 0, 77, 10)[0]
    assert nm.KEPT in whole and nm.OVER in whole and whole != nm.select(deep, 64, 0, 5, 1000, 0, 77, 10)[0]


@pytest.mark.parametrize("seed", [0, 1, 0xDEADBEEFCAFEF00D])
def test_a_quarter_of_the_units_at_four_times_the_target_is_kept(seed):
    n, target = 100000, 50
    keep, tally, _ = nm.select([(100, 1, 4 * target, 1)] * n, n, 0, 0, target, 0, seed, 255)
    kept = keep.count(nm.KEPT)
    print("seed %#x: %d of %d kept" % (seed, kept, n))
    assert abs(kept - 25000) <= 685 and keep.count(nm.OVER) == n - kept
    assert tally[:4] == [n - kept, kept, 0, 0] and tally[4 + 200] == n and tally[4 + 256 + 200] == kept


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_the_numpy_form_equals_the_plain_one(mode):
    import numpy as np
    rng = np.random.default_rng(77 + mode)
    top, seen = (1 << 31) - 1, set()
    for n_units, unit_base, target, min_cov, seed, max_bin in ((0, 0, 5, 0, 1, 3), (1, 0, 1, 0, 0, 1), (500, (1 << 32) + 5, 40, 30, 9, 64),
                                                                (500, nm.M64 - 100, top, 0, nm.M64, 65535), (300, 7, 1, 2, 1 << 63, 255)):
        n = n_units if mode == 0 else 2 * n_units
        med = np.where(rng.integers(0, 3, n) == 0, rng.integers(0, 1 << 31, n), rng.integers(0, 60, n))
        med[:n // 8] = top
        rows = np.stack([np.where(rng.integers(0, 4, n) == 0, 0, 50), np.zeros(n, np.int64), med, np.zeros(n, np.int64)], axis=1).astype(np.int32)
        keep, tally, depths = nm.select([tuple(r) for r in rows.tolist()], n_units, mode, unit_base, target, min_cov, seed, max_bin)
        k2, t2, d2 = nm.select_np(rows, n_units, mode, unit_base, target, min_cov, seed, max_bin)
        assert k2.tolist() == keep and t2.tolist() == tally and d2.tolist() == [d or 0 for d in depths]
        seen |= set(keep)
    assert seen == {nm.OVER, nm.KEPT, nm.LOW, nm.NOVALID}

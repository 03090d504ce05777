"""The saturation rule of the scan filter (M = 8) on the CPU: the numpy restatement of tests/_filter_saturation.py on random
tables and on the classes where a split of the budget can go wrong.  For every slot:
 (a) the saturations sum to at most SAT_BUDGET, (b) each lies in 0 .. QT + 1, (c) +inf entries and entries above QT + 1 take
 part as QT + 1, (d) degenerate input gives the uniform split, (e) the same input gives the same output.
"""
import numpy as np
import pytest

import _filter_saturation as fs


def _tau(T, rank_fraction, rng):
    """A threshold a query could have: the distance of a random code near the given quantile of 4000 random codes."""
    K = int(np.isfinite(T[0]).sum())
    codes = rng.integers(0, K, size=(4000, fs.M))
    d = T[np.arange(fs.M), codes].sum(axis=1, dtype=np.float64)
    return np.float32(np.sort(d)[int(rank_fraction * (len(d) - 1))])


def _check(T, key, what):
    sat = fs.saturations(T, key)
    assert len(sat) == fs.M and all(isinstance(v, int) for v in sat), what
    assert sum(sat) <= fs.SAT_BUDGET, "%s: (a) %s" % (what, sat)
    assert all(0 <= v <= fs.SAT_CAP for v in sat), "%s: (b) %s" % (what, sat)
    assert sat == fs.saturations(T.copy(), key), "%s: (e)" % what
    # (c): +inf and any finite value far above the threshold are the same input
    huge = np.where(np.isinf(T), np.float32(2.0 ** 100), T)
    if np.isinf(T).any():
        assert sat == fs.saturations(huge, key), "%s: (c) %s" % (what, sat)
    return sat


@pytest.mark.parametrize("name", fs.CLASSES)
def test_properties_on_the_classes(name):
    tables, _ = fs.class_tables(name, 12)
    rng = np.random.default_rng(5)
    for q, T in enumerate(tables):
        for frac in (0.0005, 0.02, 0.3):
            _check(T, fs.key_of(_tau(T, frac, rng)), "%s query %d quantile %g" % (name, q, frac))


def test_every_row_constant_is_uniform():
    tables, _ = fs.class_tables("constant_rows", 6)
    for T in tables:
        tau = np.float32(T[:, 0].sum(dtype=np.float64) * 1.5)                # any threshold above the one distance
        assert _check(T, fs.key_of(tau), "constant rows") == fs.uniform()    # every statistic is 0


def test_one_wide_row_does_not_pile_above_the_cap():
    tables, _ = fs.class_tables("one_wide_row", 6)
    rng = np.random.default_rng(6)
    for T in tables:
        wide = int(np.argmax(T.max(axis=1) - T.min(axis=1)))
        sat = _check(T, fs.key_of(_tau(T, 0.01, rng)), "one wide row")
        assert sat[wide] == fs.SAT_CAP
        # the constant rows share what is left, evenly (their entries are all zero: any value serves)
        rest = [v for m, v in enumerate(sat) if m != wide]
        assert max(rest) - min(rest) <= 1 and sum(sat) == fs.SAT_BUDGET


def test_two_valued_rows():
    tables, _ = fs.class_tables("two_valued", 6)
    for T in tables:
        sat = _check(T, fs.key_of(np.float32(2.0 ** 22)), "two-valued")       # two huge entries fit under the threshold
        # every row has about 128 entries at QT + 1 or beyond: equal statistics, an even split with the remainder in front
        assert sorted(sat, reverse=True) == sat and sat[0] - sat[-1] <= 1 and sum(sat) == fs.SAT_BUDGET


@pytest.mark.parametrize("name,K", [("inf_beyond_16", 16), ("inf_beyond_200", 200)])
def test_inf_rows_beyond_k(name, K):
    tables, k = fs.class_tables(name, 6)
    assert k == K and np.all(np.isinf(tables[:, :, K:])) and np.all(np.isfinite(tables[:, :, :K]))
    rng = np.random.default_rng(7)
    for T in tables:
        sat = _check(T, fs.key_of(_tau(T, 0.02, rng)), name)
        if 256 - K >= fs.RANK:                 # at least 32 entries at +inf: every statistic is QT + 1, the split is even
            assert max(sat) - min(sat) <= 1 and sum(sat) == fs.SAT_BUDGET


def test_no_scale_is_uniform():
    tables, _ = fs.class_tables("random", 4)
    for T in tables:
        B = T.min(axis=1).sum(dtype=np.float64)
        assert fs.saturations(T, fs.NO_KEY) == fs.uniform()                               # no threshold yet
        assert fs.saturations(T, fs.key_of(np.float32(B * 0.5))) == fs.uniform()          # tau' - sum of minima <= 0
        assert fs.saturations(T * np.float32(2.0 ** -140), fs.key_of(np.float32(2.0 ** -130))) == fs.uniform()  # scale > FLT_MAX
    assert fs.saturations_of_stats([0] * fs.M) == fs.uniform()


def test_threshold_so_tight_that_every_other_entry_exceeds_qt():
    tables, _ = fs.class_tables("random", 6)
    for T in tables:
        T = T.copy()
        T[:, 1:] += np.float32(4096.0)                                       # the minimum of a row stands alone
        B = T.min(axis=1).sum(dtype=np.float64)
        sat = _check(T, fs.key_of(np.float32(B + 1.0)), "tight threshold")   # span 1: every other entry is thousands of units out
        assert max(sat) - min(sat) <= 1 and sum(sat) == fs.SAT_BUDGET        # all statistics QT + 1


def test_stats_to_saturations_exhaustive_corners():
    rng = np.random.default_rng(8)
    cases = [list(rng.integers(0, fs.SAT_CAP + 1, size=fs.M)) for _ in range(3000)]
    cases += [[fs.SAT_CAP] + [0] * 7, [fs.SAT_CAP, 1] + [0] * 6, [fs.SAT_CAP] * 2 + [1] * 6, [1] * 8, [0] * 7 + [1],
              [fs.SAT_CAP] * 8, [fs.SAT_CAP, 5, 5, 5, 5, 5, 5, 5]]
    for stat in cases:
        stat = [int(v) for v in stat]
        sat = fs.saturations_of_stats(stat)
        assert sum(sat) <= fs.SAT_BUDGET and all(0 <= v <= fs.SAT_CAP for v in sat), (stat, sat)
        if any(stat):
            # nothing is wasted while a row is below the cap, and a larger statistic never gets less
            assert sum(sat) == fs.SAT_BUDGET or all(v == fs.SAT_CAP for v in sat), (stat, sat)
            for a in range(fs.M):
                for b in range(fs.M):
                    if stat[a] > stat[b]:
                        assert sat[a] >= sat[b] - 1, (stat, sat)


def test_unpack_is_the_inverse_of_slot_of_table():
    seen = sorted(fs.slot_of_table(g, c, tb) for g in range(fs.NG) for c in range(4) for tb in range(4))
    assert seen == list(range(fs.QG))
    raw = np.zeros(fs.NG * fs.M * 256 * 16 + fs.QG * 16, dtype=np.uint8)
    tab = raw[:fs.NG * fs.M * 256 * 16].reshape(fs.NG, fs.M, 256, 16)
    for g in range(fs.NG):
        for b in range(16):
            tab[g, :, :, b] = fs.slot_of_table(g, b // 4, b % 4)
    entries, sat, keys = fs.unpack_tables(raw.tobytes(), 1)
    assert np.array_equal(entries[:, 0, 0], np.arange(fs.QG)) and sat.shape == (fs.QG, 8) and keys.shape == (fs.QG,)

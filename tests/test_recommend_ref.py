"""CPU: the full-sort oracle of tests/_recommend_ref.py against ``_als_ref.recommend`` (the same statement per query), and
its candidate condition on hand-made scores."""
import numpy as np

import _als_ref as ref
import _recommend_ref as rref


def test_grid_values_are_exact():
    rng = np.random.default_rng(0)
    g = rref.grid(rng, (50, 128))
    assert rref.is_grid(g) and g.dtype == np.float32 and set(np.unique(g * 4)) == set(range(-8, 9))
    assert not rref.is_grid(np.array([0.3], np.float32)) and not rref.is_grid(np.array([2.25], np.float32))
    assert rref.is_grid(np.array([0.125], np.float32), step=8.0)
    # every score of a 128-wide grid pair is the same number in f32 and fp64 arithmetic, whatever the order
    a, b = g[:25], g[25:]
    s64 = a.astype(np.float64) @ b.astype(np.float64).T
    assert np.array_equal(s64, (a[:, ::-1] @ b[:, ::-1].T).astype(np.float64)) and np.array_equal(s64 * 16, np.round(s64 * 16))


def test_lists_equal_als_ref_recommend():
    rng = np.random.default_rng(3)
    nu, ni, D = 7, 90, 5
    X, Y = rref.grid(rng, (nu, D)), rref.grid(rng, (ni, D))           # grid values: plenty of ties
    X[2] = 0
    items = np.arange(ni) * 3 + 1
    offset = rng.integers(-4, 5, nu) * 0.25
    seen = [np.sort(rng.choice(ni, n, replace=False)) for n in (0, 1, 40, 89, 90, 3, 12)]
    rated = {u: set(items[s].tolist()) for u, s in enumerate(seen)}
    upos = np.array([4, 2, -1, 0, 6, 6, 3, 1, 5, -1, 2])
    for off in (None, offset):
        table = rref.score_table(X, Y, off)
        assert table.dtype == np.float32 and np.array_equal(table[3], ref.predict(X, Y, np.full(ni, 3), np.arange(ni), off))
        order = rref.full_order(table, items)
        for k in (1, 10, 89, 120):
            for exclude in (True, False):
                got = rref.lists(table, order, items, upos, seen if exclude else None, k)
                want = ref.recommend(X, Y, off, range(nu), items, rated, upos, k, exclude)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (k, exclude)
                assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
                assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int32
                for q, u in enumerate(upos):                          # places: where the unexcluded order holds the listed
                    if u >= 0:
                        assert np.array_equal(items[order[u][got[3][q]]], got[0][q, :got[2][q]])
    ids, _, ln, _ = rref.lists(table, order, items, upos, seen, 10)
    assert ln.tolist() == [0, 10, 0, 10, 10, 10, 1, 10, 10, 0, 10] and ids[1, :10].tolist() == \
        [i for i in items.tolist() if i not in rated[2]][:10]          # the zero row: the lowest unseen ids


def test_band_counts_on_hand_made_scores():
    # one query of X = [1], items scored 8, 7, 7, 7 - 2^-20, 6.5, 1: tau = 2 * 9 * 2^-24 * 8 = 9 * 2^-20
    X = np.array([[1.0]], np.float32)
    Y = np.array([[8.0], [7.0], [7.0], [7.0 - 2.0 ** -20], [6.5], [1.0]], np.float32)
    items, upos = np.arange(6) * 2, np.array([0, -1])
    taus = rref.tau(X, Y, upos)
    assert taus.tolist() == [9 * 2.0 ** -20, 0.0]
    table = rref.score_table(X, Y)
    order = rref.full_order(table, items)
    for k, want in ((1, 0), (2, 2), (3, 1), (4, 0), (5, 0)):
        ids, sc, ln, _ = rref.lists(table, order, items, upos, None, k)
        assert rref.band_counts(table, ids, sc, ln, items, upos, taus).tolist() == [want, 0], k
        assert rref.qualifies(table, ids, sc, ln, items, upos, taus, 1).tolist() == [want <= 1, True]
    # a seen item inside the band counts as well (never missed)
    ids, sc, ln, _ = rref.lists(table, order, items, upos, [np.array([2])], 2)
    assert ids[0].tolist() == [0, 2] and rref.band_counts(table, ids, sc, ln, items, upos, taus).tolist() == [2, 0]

"""CPU: the oracle of the implicit-feedback ALS (tests/_ials_ref.py) against first principles -- the Y^T Y identity behind the
row solve, the closed-form objective, the float32 restatement's distance to fp64, and its fit on the model the GPU test
uses."""
import numpy as np

import _als_ref as ref
import _ials_ref as iref

CHUNK, SEGMENT = 256, 512      # any geometry pins the oracle; the GPU test reads the library's own


def tiny(seed=0, nu=7, ni=9, rank=3, n=30):
    rng = np.random.default_rng(seed)
    u, i, w = iref.sum_events(rng.integers(0, nu, n), rng.integers(0, ni, n), rng.integers(1, 4, n).astype(np.float64), 2.5)
    X = rng.standard_normal((nu, rank)).astype(np.float32)
    Y = rng.standard_normal((ni, rank)).astype(np.float32)
    return u, i, w, X, Y


def test_sum_events_adds_repeats_in_fp64():
    u, i, w = iref.sum_events([2, 0, 2, 2, 0], [5, 1, 5, 3, 1], [1.0, 2.0, 0.5, 4.0, 0.25], 40.0)
    assert u.tolist() == [0, 2, 2] and i.tolist() == [1, 3, 5]
    assert w.dtype == np.float32 and w.tolist() == [90.0, 160.0, 60.0]
    u, i, w = iref.sum_events([1, 1], [0, 0], None, 3.0)
    assert w.tolist() == [6.0]


def test_row_solve_is_the_weighted_least_squares_over_all_items():
    u, i, w, _, Y = tiny()
    ni, rank = Y.shape
    G = iref.gram64(Y)
    for weighted in (True, False):
        for user in range(7):
            mine = u == user
            cols, wk = i[mine], w[mine]
            # the dense problem: EVERY item is a data point, sqrt(c) (p - x . y), and sqrt(lam) x the ridge rows
            c, p = np.ones(ni), np.zeros(ni)
            c[cols], p[cols] = 1.0 + wk.astype(np.float64), 1.0
            lam = ref.lam_of(0.1, len(cols), weighted)
            A = np.concatenate([np.sqrt(c)[:, None] * Y.astype(np.float64), np.sqrt(lam) * np.eye(rank)])
            b = np.concatenate([np.sqrt(c) * p, np.zeros(rank)])
            want = np.linalg.lstsq(A, b, rcond=None)[0]
            got = iref.solve_row64(Y, cols, wk, G, 0.1, weighted)
            if len(cols) == 0:
                assert not got.any()
                continue
            assert np.max(np.abs(got - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), (user, got, want)


def test_closed_form_objective_equals_the_dense_one():
    u, i, w, X, Y = tiny(1)
    for weighted in (True, False):
        a = iref.objective(X, Y, u, i, w, 0.1, weighted)
        b = iref.objective_dense(X, Y, u, i, w, 0.1, weighted)
        assert abs(a - b) <= 1e-10 * abs(b), (a, b)


def test_gram32_is_close_to_gram64_and_ignores_trailing_zero_rows():
    rng = np.random.default_rng(2)
    Y = rng.standard_normal((21, 5)).astype(np.float32)
    g = iref.gram32(Y, 8)
    assert g.dtype == np.float32 and np.array_equal(g, g.T)
    assert np.max(np.abs(g - iref.gram64(Y))) <= 1e-5 * np.max(np.abs(g))
    for extra in (1, 8, 9):
        assert np.array_equal(g, iref.gram32(np.concatenate([Y, np.zeros((extra, 5), np.float32)]), 8))
    assert not iref.gram32(np.zeros((0, 4), np.float32), 8).any()


def test_the_fma_argument_reaches_every_chain():
    # _als_ref's witness: fma(x, x, 2^-60), x = 1 + 2^-12, is 0x3F801001 correctly rounded and 0x3F801000 rounded twice.
    # As a chain: the row y_0 = 2^-30 leaves 2^-60, the row y_1 = x lands on the tie.
    def bits(a):
        return np.asarray(a, np.float32).view(np.uint32)
    x = np.float32(1 + 2.0 ** -12)
    Y = np.array([[2.0 ** -30], [x]], np.float32)
    one = np.ones(3, np.float32)
    for fma, want in ((ref.fma32_exact, 0x3F801001), (ref.fma32, 0x3F801000), (None, 0x3F801000)):
        kw = {} if fma is None else {"fma": fma}                               # the default is the double-rounded one
        assert bits(iref.gram32(Y, 2, **kw))[0, 0] == want
        assert bits(iref.gram32(Y, 1, **kw))[0, 0] == 0x3F801000               # two segments: the fp64 sum, rounded once
        A, b = iref.gram_rhs32(Y, [0, 1], one, 2, **kw)                        # w = 1: fl32(w y) = y
        assert bits(A)[0, 0] == want
        # right-hand side, c = 1 + w: the even chain is 1 * 2^-60, then (after an odd entry on a zero row) x * x, w = x - 1
        w = np.float32([0.0, 0.0, x - 1])
        assert np.float32(1) + w[2] == x
        A, b = iref.gram_rhs32(np.array([[2.0 ** -60], [x], [0.0]], np.float32), [0, 2, 1], w, 4, **kw)
        assert bits(b)[0] == want
    # solve_row32 hands the argument on to both halves: the explicit witness matrix of test_als_ref through G32
    G = np.array([[1.0, 0.0], [-x, 4.0]], np.float32)
    Yz = np.zeros((1, 2), np.float32)                                          # a zero factor row: A = 0, b = 0
    part = (np.zeros((2, 2), np.float32), np.float32([x, 2.0 ** -60]))
    xe = iref.solve_row32(Yz, [0], one[:1], G, 1e-30, False, 4, partial=part, fma=ref.fma32_exact)
    xd = iref.solve_row32(Yz, [0], one[:1], G, 1e-30, False, 4, partial=part)
    assert np.array_equal(bits(xe), bits(ref.cholesky_solve32(G, part[1], np.float32(1e-30), ref.fma32_exact)))
    assert bits(xe)[1] != bits(xd)[1]


def test_float32_row_solve_is_close_to_fp64():
    rng = np.random.default_rng(3)
    for rank, n_other, n in ((3, 9, 4), (8, 60, 37), (33, 97, 300)):
        Y = (rng.standard_normal((n_other, rank)) / np.sqrt(rank)).astype(np.float32)
        cols = rng.integers(0, n_other, n)
        w = (rng.integers(1, 41, n) * 0.5).astype(np.float32)
        for weighted in (True, False):
            x64 = iref.solve_row64(Y, cols, w, iref.gram64(Y), 0.1, weighted)
            x32 = iref.solve_row32(Y, cols, w, iref.gram32(Y, 16), 0.1, weighted, 16)
            assert x32.dtype == np.float32
            assert np.max(np.abs(x32 - x64)) <= 1e-4 * np.max(np.abs(x64)), (rank, weighted)
    assert not iref.solve_row32(Y, [], [], iref.gram32(Y, 16), 0.1, True, 16).any()


def test_fold_in_drops_unknown_ids_and_adds_repeats():
    rng = np.random.default_rng(5)
    items = np.array([2, 4, 6, 8, 10])
    Y = rng.standard_normal((5, 2)).astype(np.float32)
    X, d, i = iref.fold_in(Y, items, [4, 3, 4, 10, 7, 7, 2], [0, 4, 4, 6, 7], 2.0, 0.1, False, CHUNK, SEGMENT)
    assert d.tolist() == [0, 0, 3] and i.tolist() == [1, 4, 0]
    assert X.shape == (4, 2) and not X[1].any() and not X[2].any()              # empty, and only unknown ids
    G = iref.gram32(Y, SEGMENT)
    assert np.array_equal(X[0], iref.solve_row32(Y, [1, 4], np.float32([4.0, 2.0]), G, 0.1, False, CHUNK))
    assert np.array_equal(X[3], iref.solve_row32(Y, [0], np.float32([2.0]), G, 0.1, False, CHUNK))


def test_float32_fit_of_the_small_model_does_not_increase():
    user, item = iref.small_events()
    users, upos = np.unique(user, return_inverse=True)
    items, ipos = np.unique(item, return_inverse=True)
    u, i, w = iref.sum_events(upos, ipos, None, iref.SMALL["alpha"])
    assert len(u) < 4000                                                           # the events do repeat
    Y0 = iref.initial_items(len(items), iref.SMALL["rank"])
    X, Y, history = iref.fit(u, i, w, Y0, iref.SMALL["reg"], iref.SMALL["weighted_reg"], iref.SMALL_HALF_SWEEPS, CHUNK,
                             SEGMENT)
    assert X.dtype == Y.dtype == np.float32 and len(history) == iref.SMALL_HALF_SWEEPS
    for a, b in zip(history, history[1:]):
        assert b <= a * (1 + 1e-6), history
    assert history[-1] < 0.9 * history[0]
    # and it tracks the fp64 fit
    _, _, h64 = iref.fit(u, i, w, Y0, iref.SMALL["reg"], iref.SMALL["weighted_reg"], iref.SMALL_HALF_SWEEPS)
    assert abs(history[-1] - h64[-1]) <= 1e-3 * h64[-1], (history, h64)

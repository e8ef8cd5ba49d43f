"""CPU: pins the ALS oracle (tests/_als_ref.py) -- a hand-worked 2 x 2 example with a closed-form minimiser, the normal
equations in fp64, and the monotone descent of the fp64 objective."""
import numpy as np

import _als_ref as ref


zipf_ratings = ref.zipf_ratings


def test_hand_worked_two_by_two():
    # Y = [[1, 2], [3, 4]], d = [1, 2], reg = 1 weighted (lam = 2):  A = Y^T Y + 2 I = [[12, 14], [14, 22]], det = 68,
    # b = 1 * (1, 2) + 2 * (3, 4) = (7, 10),  x = A^-1 b = (22 * 7 - 14 * 10, -14 * 7 + 12 * 10) / 68 = (14, 22) / 68
    Y = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
    want = np.array([14.0, 22.0]) / 68.0
    x64 = ref.solve_row64(Y, [0, 1], [1.0, 2.0], 1.0, True)
    assert np.allclose(x64, want, rtol=1e-14, atol=0)
    x32 = ref.solve_row32(Y, [0, 1], np.float32([1.0, 2.0]), 1.0, True, chunk=2)
    assert x32.dtype == np.float32 and np.allclose(x32, want, rtol=1e-6, atol=0)
    G, b = ref.gram_rhs32(Y, [0, 1], np.float32([1.0, 2.0]), chunk=1)       # two chunks of one rating: the same exact sums
    assert np.array_equal(G, [[10, 14], [14, 20]]) and np.array_equal(b, [7, 10])
    # unweighted: lam = 1, A = [[11, 14], [14, 21]], det = 35, x = (21 * 7 - 140, -98 + 110) / 35 = (7, 12) / 35
    assert np.allclose(ref.solve_row64(Y, [0, 1], [1.0, 2.0], 1.0, False), np.array([7.0, 12.0]) / 35.0, rtol=1e-14, atol=0)
    assert np.array_equal(ref.solve_row64(Y, [], [], 1.0, True), [0, 0])
    assert np.array_equal(ref.solve_row32(Y, [], [], 1.0, True, 2), [0, 0])


def test_normal_equations_hold_in_fp64():
    rng = np.random.default_rng(5)
    for rank, n, weighted, reg in ((1, 1, True, 0.1), (5, 3, False, 1e-3), (32, 7, True, 0.1), (33, 200, False, 1e-3),
                                   (64, 40, True, 1e-3)):
        Y = (rng.standard_normal((50, rank)) / np.sqrt(rank)).astype(np.float32)
        cols = rng.integers(0, 50, n)
        d = (rng.integers(-8, 9, n) * 0.5).astype(np.float32)
        x = ref.solve_row64(Y, cols, d, reg, weighted)
        y = Y[cols].astype(np.float64)
        A = y.T @ y + ref.lam_of(reg, n, weighted) * np.eye(rank)
        b = y.T @ d.astype(np.float64)
        assert np.max(np.abs(A @ x - b)) <= 1e-12 * max(np.max(np.abs(b)), np.max(np.abs(A)) * np.max(np.abs(x)))
        x32 = ref.solve_row32(Y, cols, d, reg, weighted, chunk=16)
        assert np.max(np.abs(x32 - x)) <= 2e-3 * np.max(np.abs(x))             # the restatement solves the same system


def test_restatement_fails_on_a_nan_factor():
    Y = np.array([[1.0, np.nan], [3.0, 4.0]], np.float32)
    assert ref.solve_row32(Y, [0, 1], np.float32([1.0, 2.0]), 0.1, True, 2) is None


def test_fp64_objective_never_increases():
    rng = np.random.default_rng(11)
    u, i, r = zipf_ratings(rng, 40, 25, 300)
    users, upos = np.unique(u, return_inverse=True)
    items, ipos = np.unique(i, return_inverse=True)
    mean = np.bincount(upos, weights=r) / np.bincount(upos)
    d = r - mean[upos]
    for weighted in (True, False):
        Y0 = rng.standard_normal((len(items), 4)) * 0.5
        _, _, history = ref.fit(upos, ipos, d, Y0, 0.1, weighted, 6)
        assert len(history) == 6
        assert all(b <= a * (1 + 1e-12) for a, b in zip(history, history[1:])), history


def test_predict_residuals_and_recommend_agree():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((4, 3)).astype(np.float32)
    Y = rng.standard_normal((6, 3)).astype(np.float32)
    c = np.array([3.0, 2.5, 4.0, 1.0])
    p = ref.predict(X, Y, [0, 1, -1, 3], [5, 0, 2, -1], c)
    assert p.dtype == np.float32 and np.isnan(p[2]) and np.isnan(p[3])
    assert p[0] == np.float32(c[0] + sum(np.float64(X[0, k]) * np.float64(Y[5, k]) for k in range(3)))
    res = ref.residuals(X, Y, [0, 1], [5, 0], np.float32([1.0, -0.5]))
    assert res[1] == np.float32(np.float64(-0.5) - ref.dot64(X, Y, np.array([1]), np.array([0]))[0])
    users, items = [10, 20, 30, 40], np.array([1, 2, 3, 5, 8, 13])
    ids, sc, ln = ref.recommend(X, Y, c, users, items, {20: {1, 2, 3, 5, 8, 13}, 10: {3}}, [10, 20, 99], 4)
    assert list(ln) == [4, 0, 0] and 3 not in ids[0] and np.all(ids[1:] == -1)
    assert np.all(np.diff(sc[0].astype(np.float64)) <= 0)
    assert sc[0, 0] == ref.predict(X, Y, [0], [list(items).index(ids[0, 0])], c)[0]

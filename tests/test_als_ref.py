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


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def fma_triples():
    """A few thousand float32 triples: random ones, ones whose product nearly cancels c, and ones whose c is far below the
    product's last bit (the double-rounded emulation's weak spot)."""
    rng = np.random.default_rng(17)
    n = 1500
    a = (rng.standard_normal(3 * n) * np.exp2(rng.integers(-20, 21, 3 * n))).astype(np.float32)
    b = (rng.standard_normal(3 * n) * np.exp2(rng.integers(-20, 21, 3 * n))).astype(np.float32)
    c = (rng.standard_normal(3 * n) * np.exp2(rng.integers(-20, 21, 3 * n))).astype(np.float32)
    prod = a.astype(np.float64) * b.astype(np.float64)
    c[n:2 * n] = (-prod[n:2 * n] * (1 + rng.integers(-3, 4, n) * 2.0 ** -24)).astype(np.float32)   # cancelling
    # a product on a float32 tie (1 + 2^-12)^2 style, and a c too small for fp64 to see beside it
    m = rng.integers(1, 2 ** 11, n).astype(np.float64)
    a[2 * n:] = b[2 * n:] = (1 + (2 * m + 1) * 2.0 ** -12).astype(np.float32)
    c[2 * n:] = (rng.choice([-1.0, 1.0], n) * np.exp2(-rng.integers(40, 90, n).astype(np.float64))).astype(np.float32)
    return a, b, c


def fma_rational(a, b, c):
    """The float32 nearest (ties to even) to a * b + c in exact rational arithmetic, one triple; normal range only."""
    from fractions import Fraction
    v = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if v == 0:
        return np.float32(0.0)
    sign, v = (-1, -v) if v < 0 else (1, v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1                                       # 2^e <= v < 2^(e + 1)
    assert -126 <= e <= 126
    q = v / Fraction(2) ** (e - 23)                  # in [2^23, 2^24): round it to an integer, ties to even
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n & 1):
        n += 1
    return np.float32(sign * float(Fraction(n) * Fraction(2) ** (e - 23)))


def test_fma32_exact_is_the_correctly_rounded_fma():
    a, b, c = fma_triples()
    got = ref.fma32_exact(a, b, c)
    assert got.dtype == np.float32 and got.shape == a.shape
    want = np.array([fma_rational(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(bits(got), bits(want))
    assert np.any(bits(ref.fma32(a, b, c)) != bits(want))                    # the triples do reach the double rounding
    # the witness: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 tie; c = 2^-60 breaks it upward, and fp64 cannot see c
    x, z = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    assert bits(ref.fma32_exact(x, x, z)) == 0x3F801001 and bits(ref.fma32(x, x, z)) == 0x3F801000
    assert bits(ref.fma32_exact(x, x, -z)) == 0x3F801000 and bits(fma_rational(x, x, z)) == 0x3F801001
    # shapes broadcast, and what is not finite stays so
    assert ref.fma32_exact(np.ones((3, 1), np.float32), np.ones((1, 4), np.float32), np.float32(2.0)).shape == (3, 4)
    assert np.isnan(ref.fma32_exact(np.float32(np.nan), 1.0, 1.0)) and np.isposinf(ref.fma32_exact(3e38, 3e38, 1.0))
    assert ref.fma32_exact(np.float32(np.inf), 1.0, 1.0) == np.inf


def test_both_fmas_agree_on_the_hand_worked_cases():
    Y = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
    d = np.float32([1.0, 2.0])
    for chunk in (1, 2):
        G, b = ref.gram_rhs32(Y, [0, 1], d, chunk, fma=ref.fma32_exact)
        assert np.array_equal(G, [[10, 14], [14, 20]]) and np.array_equal(b, [7, 10])
    for weighted in (True, False):
        x = ref.solve_row32(Y, [0, 1], d, 1.0, weighted, 2)
        xe = ref.solve_row32(Y, [0, 1], d, 1.0, weighted, 2, fma=ref.fma32_exact)
        assert xe.dtype == np.float32 and np.array_equal(bits(x), bits(xe))
    assert np.array_equal(ref.solve_row32(Y, [], [], 1.0, True, 2, fma=ref.fma32_exact), [0, 0])
    Yn = np.array([[1.0, np.nan], [3.0, 4.0]], np.float32)
    assert ref.solve_row32(Yn, [0, 1], d, 0.1, True, 2, fma=ref.fma32_exact) is None


def test_the_fma_argument_reaches_every_chain():
    # the witness as a Gram chain: y_0 = 2^-30 leaves 2^-60, y_1 = 1 + 2^-12 lands on the tie
    x = np.float32(1 + 2.0 ** -12)
    Y = np.array([[2.0 ** -30], [x]], np.float32)
    for fma, want in ((ref.fma32_exact, 0x3F801001), (ref.fma32, 0x3F801000), (None, 0x3F801000)):
        kw = {} if fma is None else {"fma": fma}                               # the default is the double-rounded one
        G, b = ref.gram_rhs32(Y, [0, 1], np.float32([2.0 ** -30, x]), 2, **kw)
        assert bits(G)[0, 0] == want
        G, b = ref.gram_rhs32(Y, [0, 0, 1], np.float32([2.0 ** -30, 0, x]), 4, **kw)    # even chain: the witness; odd: 0
        assert bits(b)[0] == want
        # ... and as the forward solve: L = [[1, 0], [-x, .]], z_0 = x, z_1 = fma(x, x, 2^-60) / l_11
        A = np.array([[1.0, 0.0], [-x, 4.0]], np.float32)
        z = ref.cholesky_solve32(A, np.float32([x, 2.0 ** -60]), 0.0, **kw)
        l11 = np.sqrt(ref.fma32_exact(x, -x, np.float32(4.0)), dtype=np.float32)
        x1 = np.float32(np.float32(np.array([want], np.uint32).view(np.float32)[0] / l11) / l11)
        assert bits(z)[1] == bits(x1)


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

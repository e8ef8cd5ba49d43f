"""CPU restatement of esrecsys_amd/factorization.py and esr_als.hip in NumPy: the oracle of the GPU tests, pinned itself by
test_als_ref.py.

Two row solvers.  ``solve_row64`` is the reference: ``numpy.linalg.solve`` on the fp64 Gram of the float32 factors.
``solve_row32`` restates the kernel's arithmetic in float32 -- chunked k-ordered accumulation, Cholesky, two triangular
solves, in the kernel's stated order -- to measure what float32 itself costs on a given row.  A float32 fma is emulated as
``float32(float64(a) * float64(b) + float64(c))``: the product is exact in a double, the sum rounds twice (to 53, then to 24
bits), which differs from a true fma in rare last-bit cases only.  That is the default (``fma32``), and what the bound tests
measure with.  ``fma32_exact`` is the correctly rounded float32 fma; every float32 function here takes it as ``fma=`` and
the bit-for-bit tests (test_gpu_als_exact.py) run on it.

lam: the C ABI takes ``reg`` as a float, so both solvers use ``float64(float32(reg))``; the float32 one multiplies by the
row's count in float32 as the kernel does."""
import numpy as np

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def fma32_exact(a, b, c):
    """The correctly rounded float32 fma, vectorised.  The product of two float32 is exact in fp64; TwoSum of it and c gives
    the fp64 sum s and its exact error e; s is rounded to odd (where e != 0 and the last bit of s is even, one fp64 ulp
    toward e's sign), and a sum rounded to odd at 53 >= 24 + 2 bits rounds to float32 as the exact sum does."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.asarray(c, F32).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        v = s - p
        e = (p - (s - v)) + (c - v)
        even = (np.ascontiguousarray(s).view(np.uint64) & np.uint64(1)) == 0
        step = np.isfinite(s) & np.isfinite(e) & (e != 0) & even
        s = np.where(step, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def lam_of(reg, n, weighted):
    return F64(F32(reg)) * (F64(n) if weighted else F64(1.0))


def solve_row64(Y, cols, d, reg, weighted):
    """The fp64 solution of (sum y y^T + lam I) x = sum d y over the row's ratings; zeros for an empty row."""
    rank = Y.shape[1]
    if len(cols) == 0:
        return np.zeros(rank, F64)
    y = Y[np.asarray(cols)].astype(F64)
    A = y.T @ y + lam_of(reg, len(cols), weighted) * np.eye(rank)
    return np.linalg.solve(A, y.T @ np.asarray(d, F64))


def gram_rhs32(Y, cols, d, chunk, fma=fma32):
    """(G float32[rank, rank], b float32[rank]) in the kernel's order: per chunk of `chunk` consecutive ratings the Gram
    entries are a k-ordered fma chain from 0 and the right-hand side is the chain over the chunk's even ratings plus the
    chain over its odd ones; chunk partials are added in ascending chunk order."""
    rank = Y.shape[1]
    G = b = None
    for c0 in range(0, len(cols), chunk):
        g = np.zeros((rank, rank), F32)
        r = [np.zeros(rank, F32), np.zeros(rank, F32)]
        for k in range(c0, min(c0 + chunk, len(cols))):
            y = Y[cols[k]]
            g = fma(y[:, None], y[None, :], g)
            r[(k - c0) & 1] = fma(F32(d[k]), y, r[(k - c0) & 1])
        p = (r[0] + r[1]).astype(F32)
        G, b = (g, p) if G is None else ((G + g).astype(F32), (b + p).astype(F32))
    return G, b


def cholesky_solve32(G, b, lam, fma=fma32):
    """x float32 of (G + lam I) x = b: left-looking float32 Cholesky and two column-oriented solves; None where a pivot is
    not finite and positive.  Only the lower triangle of G is read."""
    n = G.shape[0]
    L = G.astype(F32).copy()
    L[np.arange(n), np.arange(n)] = (np.diag(L) + F32(lam)).astype(F32)
    for j in range(n):
        s = L[j:, j].copy()
        for k in range(j):
            s = fma(-L[j:, k], L[j, k], s)
        if not (s[0] > 0 and np.isfinite(s[0])):
            return None
        dj = np.sqrt(s[0], dtype=F32)
        L[j, j] = dj
        L[j + 1:, j] = (s[1:] / dj).astype(F32)
    x = np.asarray(b, F32).copy()
    for j in range(n):
        x[j] = F32(x[j] / L[j, j])
        x[j + 1:] = fma(-L[j + 1:, j], x[j], x[j + 1:])
    for j in range(n - 1, -1, -1):
        x[j] = F32(x[j] / L[j, j])
        x[:j] = fma(-L[j, :j], x[j], x[:j])
    return x


def lam32(reg, n, weighted):
    return F32(F32(reg) * F32(n)) if weighted else F32(reg)


def solve_row32(Y, cols, d, reg, weighted, chunk, gram=None, fma=fma32):
    """The float32 restatement of one row (``gram``: a cached gram_rhs32 of the same row)."""
    if len(cols) == 0:
        return np.zeros(Y.shape[1], F32)
    G, b = gram_rhs32(Y, cols, d, chunk, fma) if gram is None else gram
    return cholesky_solve32(G, b, lam32(reg, len(cols), weighted), fma)


def half_sweep(Y, offsets, cols, d, reg, weighted, chunk=None):
    """All rows of a CSR: float64 [n_rows, rank] by solve_row64, or float32 by solve_row32 when `chunk` is given."""
    n_rows = len(offsets) - 1
    out = np.zeros((n_rows, Y.shape[1]), F64 if chunk is None else F32)
    for r in range(n_rows):
        a, e = int(offsets[r]), int(offsets[r + 1])
        out[r] = (solve_row64(Y, cols[a:e], d[a:e], reg, weighted) if chunk is None
                  else solve_row32(Y, cols[a:e], d[a:e], reg, weighted, chunk))
    return out


def dot64(X, Y, upos, ipos):
    """sum_d float64(x[d]) * float64(y[d]) in ascending d from 0."""
    acc = np.zeros(len(upos), F64)
    for k in range(X.shape[1]):
        acc = acc + X[upos, k].astype(F64) * Y[ipos, k].astype(F64)
    return acc


def predict(X, Y, upos, ipos, offset=None):
    """float32(c[u] + dot) per pair; NaN where a position is negative."""
    upos, ipos = np.asarray(upos, np.int64), np.asarray(ipos, np.int64)
    ok = (upos >= 0) & (ipos >= 0)
    u, i = np.where(ok, upos, 0), np.where(ok, ipos, 0)
    acc = dot64(X, Y, u, i)
    if offset is not None:
        acc = np.asarray(offset, F64)[u] + acc
    return np.where(ok, acc.astype(F32), F32(np.nan)).astype(F32)


def residuals(X, Y, upos, ipos, d):
    return (np.asarray(d, F32).astype(F64) - dot64(X, Y, np.asarray(upos, np.int64), np.asarray(ipos, np.int64))).astype(F32)


def objective(X, Y, upos, ipos, d, reg, weighted, res=None):
    """J in fp64 from the float32 residuals (or from exact fp64 ones when X is float64)."""
    upos, ipos = np.asarray(upos, np.int64), np.asarray(ipos, np.int64)
    if res is None:
        res = (residuals(X, Y, upos, ipos, d) if X.dtype == F32
               else np.asarray(d, F64) - np.einsum("qk,qk->q", X[upos], Y[ipos]))
    wu = np.bincount(upos, minlength=X.shape[0]).astype(F64) if weighted else np.ones(X.shape[0])
    wi = np.bincount(ipos, minlength=Y.shape[0]).astype(F64) if weighted else np.ones(Y.shape[0])
    res = np.asarray(res, F64)
    return float((res * res).sum() + reg * (wu * (X.astype(F64) ** 2).sum(1)).sum()
                 + reg * (wi * (Y.astype(F64) ** 2).sum(1)).sum())


def csr(major, minor, n_major):
    """(offsets int64[n_major + 1], order): rows sorted by (major, minor)."""
    order = np.lexsort((minor, major))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(major, minlength=n_major))]).astype(np.int64)
    return offsets, order


def fit(upos, ipos, d, Y0, reg, weighted, half_sweeps, chunk=None):
    """ALS from item factors Y0 (user side solved first): (X, Y, [objective after every half-sweep]).  fp64 arithmetic, or
    the float32 restatement when `chunk` is given."""
    upos, ipos = np.asarray(upos, np.int64), np.asarray(ipos, np.int64)
    dt = F64 if chunk is None else F32
    d = np.asarray(d, dt)
    nu, ni = int(upos.max()) + 1, Y0.shape[0]
    uo, uorder = csr(upos, ipos, nu)
    io, iorder = csr(ipos, upos, ni)
    X, Y = np.zeros((nu, Y0.shape[1]), dt), Y0.astype(dt)
    history = []
    for h in range(half_sweeps):
        if h % 2 == 0:
            X = half_sweep(Y, uo, ipos[uorder], d[uorder], reg, weighted, chunk).astype(dt)
        else:
            Y = half_sweep(X, io, upos[iorder], d[iorder], reg, weighted, chunk).astype(dt)
        history.append(objective(X, Y, upos, ipos, d, reg, weighted))
    return X, Y, history


def zipf_ratings(rng, nu, ni, nnz):
    """(user, item, rating): `nnz` distinct pairs with Zipf item popularity and half-star ratings, in random order."""
    p = 1.0 / np.arange(1, ni + 1)
    pairs = set()
    while len(pairs) < nnz:
        u = rng.integers(0, nu, nnz)
        i = rng.choice(ni, nnz, p=p / p.sum())
        pairs.update(zip(u.tolist(), i.tolist()))
    pairs = np.array(sorted(pairs))[rng.permutation(len(pairs))[:nnz]]
    return pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64), rng.integers(1, 11, nnz) * 0.5


def recommend(X, Y, offset, users, items, rated, query_users, k, exclude_rated=True):
    """By full sort: per query user every item scored by ``predict``, the user's own items removed, ordered by (score
    descending, item id ascending), cut to k.  `rated`: {user id: set of item ids}.  (ids [nq, k] padded with -1, scores
    padded with 0, lengths)."""
    users, items = list(users), np.asarray(items)
    nq, ni = len(query_users), len(items)
    ids = np.full((nq, k), -1, np.int32)
    scores = np.zeros((nq, k), F32)
    lengths = np.zeros(nq, np.int32)
    where = {u: p for p, u in enumerate(users)}
    for q, u in enumerate(query_users):
        if int(u) not in where:
            continue
        p = where[int(u)]
        sc = predict(X, Y, np.full(ni, p), np.arange(ni), offset)
        keep = np.ones(ni, bool)
        if exclude_rated:
            keep = ~np.isin(items, list(rated.get(int(u), ())))
        cand = np.nonzero(keep)[0]
        order = cand[np.lexsort((items[cand], -sc[cand].astype(F64)))][:k]
        ids[q, :len(order)] = items[order]
        scores[q, :len(order)] = sc[order]
        lengths[q] = len(order)
    return ids, scores, lengths

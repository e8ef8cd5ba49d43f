"""CPU restatement of the implicit-feedback path of esrecsys_amd/factorization.py (ImplicitALS) and esr_als.hip in NumPy:
the oracle of test_gpu_ials.py, pinned itself by test_ials_ref.py.

Model (Hu, Koren, Volinsky 2008).  Every (user, item) cell is fitted: preference 1 on the seen cells and 0 elsewhere,
confidence 1 + w on the seen cells (w float32) and 1 elsewhere.  A row with n seen cells solves

    (G + sum_k w_k y_k y_k^T + lam I) x = sum_k c_k y_k,     G = Y^T Y,   c_k = 1 + w_k,   lam = reg * (n if weighted else 1).

Arithmetic order of the float32 restatement, as esr_als.hip states it:
  gram32       the table is cut into segments of `segment` consecutive rows; a segment's entry is ONE k-ordered float32 fma
               chain from 0; the segment partials are added per entry in fp64 in ascending segment order and rounded once.
  solve_row32  (1) the entries in CSR order, cut into chunks of `chunk`; (2) within a chunk the entry (i, j) is the k-ordered
               chain acc = fma32(fl32(w_k * y_k[i]), y_k[j], acc) from 0 (the row index carries the weight: only the lower
               triangle i >= j is read afterwards); (3) the right-hand side is fma32(c_k, y_k[d], acc), c_k = fl32(1 + w_k),
               over the chunk's even entries plus the same chain over its odd ones; (4) chunk partials are added in ascending
               order in float32; (5) then G[i][j] is added; (6) then lam on the diagonal; (7) then _als_ref.cholesky_solve32.
fma32 is _als_ref's double-rounded emulation, the default; ``fma=_als_ref.fma32_exact`` runs the same steps on the correctly
rounded float32 fma (the bit-for-bit tests do).
"""
import numpy as np

import _als_ref as ref
from _als_ref import F32, F64, fma32


def gram64(Y):
    y = np.asarray(Y, F64)
    return y.T @ y


def gram32(Y, segment, fma=fma32):
    Y = np.asarray(Y, F32)
    rank = Y.shape[1]
    total = np.zeros((rank, rank), F64)
    for s0 in range(0, len(Y), segment):
        g = np.zeros((rank, rank), F32)
        for k in range(s0, min(s0 + segment, len(Y))):
            g = fma(Y[k][:, None], Y[k][None, :], g)
        total = total + g.astype(F64)
    return total.astype(F32)


def solve_row64(Y, cols, w, G64, reg, weighted):
    """numpy.linalg.solve on the fp64 system of the float32 factors, the float32 weights and the fp64 Gram; zeros for an
    empty row."""
    rank = Y.shape[1]
    if len(cols) == 0:
        return np.zeros(rank, F64)
    y = Y[np.asarray(cols)].astype(F64)
    w = np.asarray(w, F32).astype(F64)
    A = np.asarray(G64, F64) + (y * w[:, None]).T @ y + ref.lam_of(reg, len(cols), weighted) * np.eye(rank)
    return np.linalg.solve(A, y.T @ (1.0 + w))


def gram_rhs32(Y, cols, w, chunk, fma=fma32):
    """(sum_k w_k y_k y_k^T float32[rank, rank], sum_k c_k y_k float32[rank]): steps (1) to (4) of the module text."""
    rank = Y.shape[1]
    A = b = None
    for c0 in range(0, len(cols), chunk):
        g = np.zeros((rank, rank), F32)
        r = [np.zeros(rank, F32), np.zeros(rank, F32)]
        for k in range(c0, min(c0 + chunk, len(cols))):
            y = Y[cols[k]]
            wk = F32(w[k])
            g = fma((wk * y).astype(F32)[:, None], y[None, :], g)
            r[(k - c0) & 1] = fma(F32(F32(1.0) + wk), y, r[(k - c0) & 1])
        p = (r[0] + r[1]).astype(F32)
        A, b = (g, p) if A is None else ((A + g).astype(F32), (b + p).astype(F32))
    return A, b


def solve_row32(Y, cols, w, G32, reg, weighted, chunk, partial=None, fma=fma32):
    """The float32 restatement of one row (``partial``: a cached gram_rhs32 of the same row); None where a pivot fails."""
    if len(cols) == 0:
        return np.zeros(Y.shape[1], F32)
    A, b = gram_rhs32(Y, cols, w, chunk, fma) if partial is None else partial
    A = (A + np.asarray(G32, F32)).astype(F32)
    return ref.cholesky_solve32(A, b, ref.lam32(reg, len(cols), weighted), fma)


def half_sweep(Y, offsets, cols, w, reg, weighted, chunk=None, segment=None):
    """All rows of a CSR: float64 by solve_row64, or float32 by gram32 + solve_row32 when `chunk` and `segment` are given."""
    n_rows = len(offsets) - 1
    f32 = chunk is not None
    G = gram32(Y, segment) if f32 else gram64(Y)
    out = np.zeros((n_rows, Y.shape[1]), F32 if f32 else F64)
    for r in range(n_rows):
        a, e = int(offsets[r]), int(offsets[r + 1])
        out[r] = (solve_row32(Y, cols[a:e], w[a:e], G, reg, weighted, chunk) if f32
                  else solve_row64(Y, cols[a:e], w[a:e], G, reg, weighted))
    return out


def sum_events(major, minor, strength, alpha):
    """Distinct (major, minor) pairs sorted by (major, minor) and w = float32(alpha * the strengths summed in fp64 in the
    events' order)."""
    major, minor = np.asarray(major, np.int64), np.asarray(minor, np.int64)
    strength = np.ones(len(major), F64) if strength is None else np.asarray(strength, F64)
    order = np.lexsort((minor, major))           # stable: equal pairs keep the events' order
    key = (major[order] << 32) | minor[order]
    ukey, starts = np.unique(key, return_index=True)
    sums = np.add.reduceat(strength[order], starts) if len(key) else np.zeros(0, F64)
    return ukey >> 32, ukey & 0xFFFFFFFF, (F64(alpha) * sums).astype(F32)


def objective_dense(X, Y, upos, ipos, w, reg, weighted):
    """sum over ALL cells of c (p - x . y)^2 + reg (sum w_u |x_u|^2 + sum w_i |y_i|^2) with the matrices written out."""
    X64, Y64 = np.asarray(X, F64), np.asarray(Y, F64)
    upos, ipos = np.asarray(upos, np.int64), np.asarray(ipos, np.int64)
    P = np.zeros((len(X64), len(Y64)))
    C = np.ones((len(X64), len(Y64)))
    P[upos, ipos] = 1.0
    C[upos, ipos] = 1.0 + np.asarray(w, F32).astype(F64)
    wu = np.bincount(upos, minlength=len(X64)).astype(F64) if weighted else np.ones(len(X64))
    wi = np.bincount(ipos, minlength=len(Y64)).astype(F64) if weighted else np.ones(len(Y64))
    return float((C * (P - X64 @ Y64.T) ** 2).sum() + reg * (wu * (X64 ** 2).sum(1)).sum() + reg * (wi * (Y64 ** 2).sum(1)).sum())


def objective(X, Y, upos, ipos, w, reg, weighted):
    """The same number without the matrix: sum_u x_u^T (Y^T Y) x_u over all cells at confidence 1 and preference 0, and
    (1 + w) (1 - s)^2 - s^2 more on a seen cell with dot s."""
    X64, Y64 = np.asarray(X, F64), np.asarray(Y, F64)
    upos, ipos = np.asarray(upos, np.int64), np.asarray(ipos, np.int64)
    s = np.einsum("qk,qk->q", X64[upos], Y64[ipos])
    c = 1.0 + np.asarray(w, F32).astype(F64)
    wu = np.bincount(upos, minlength=len(X64)).astype(F64) if weighted else np.ones(len(X64))
    wi = np.bincount(ipos, minlength=len(Y64)).astype(F64) if weighted else np.ones(len(Y64))
    return float(((X64 @ (Y64.T @ Y64)) * X64).sum() + (c * (1.0 - s) ** 2 - s * s).sum()
                 + reg * (wu * (X64 ** 2).sum(1)).sum() + reg * (wi * (Y64 ** 2).sum(1)).sum())


def fit(upos, ipos, w, Y0, reg, weighted, half_sweeps, chunk=None, segment=None):
    """ALS over distinct pairs (upos, ipos, w) from item factors Y0, the user side first: (X, Y, [objective after every
    half-sweep]); fp64, or the float32 restatement when `chunk` and `segment` are given."""
    upos, ipos = np.asarray(upos, np.int64), np.asarray(ipos, np.int64)
    w = np.asarray(w, F32)
    dt = F64 if chunk is None else F32
    nu, ni = int(upos.max()) + 1, Y0.shape[0]
    uo, uorder = ref.csr(upos, ipos, nu)
    io, iorder = ref.csr(ipos, upos, ni)
    X, Y = np.zeros((nu, Y0.shape[1]), dt), Y0.astype(dt)
    history = []
    for h in range(half_sweeps):
        if h % 2 == 0:
            X = half_sweep(Y, uo, ipos[uorder], w[uorder], reg, weighted, chunk, segment).astype(dt)
        else:
            Y = half_sweep(X, io, upos[iorder], w[iorder], reg, weighted, chunk, segment).astype(dt)
        history.append(objective(X, Y, upos, ipos, w, reg, weighted))
    return X, Y, history


def fold_in(Y, items, indices, doc_offsets, alpha, reg, weighted, chunk, segment, strengths=None):
    """float32[ndocs, rank] of new id documents against the item factors Y of the ascending ids `items`: unknown ids are
    dropped, repeats add up, a document without a known id gets zeros.  Also the (doc, item position) pairs it used."""
    items = np.asarray(items, np.int64)
    indices, off = np.asarray(indices, np.int64), np.asarray(doc_offsets, np.int64)
    docs = np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))
    pos = np.searchsorted(items, indices).clip(max=len(items) - 1)
    known = items[pos] == indices
    s = None if strengths is None else np.asarray(strengths, F64)[known]
    d, i, w = sum_events(docs[known], pos[known], s, alpha)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(d, minlength=len(off) - 1))]).astype(np.int64)
    return half_sweep(np.asarray(Y, F32), offsets, i, w, reg, weighted, chunk, segment), d, i


def zipf_events(rng, nu, ni, n):
    """(user, item): `n` events with Zipf item popularity; a pair may repeat."""
    p = 1.0 / np.arange(1, ni + 1)
    return rng.integers(0, nu, n).astype(np.int64), rng.choice(ni, n, p=p / p.sum()).astype(np.int64)


def recommend(X, Y, users, items, seen, query_users, k, exclude_seen=True):
    """The full-sort recommender of _als_ref without an offset: every item scored by ``predict``, the seen ones removed,
    ordered by (score descending, item id ascending), cut to k.  `seen`: {user id: set of item ids}."""
    return ref.recommend(X, Y, None, users, items, seen, query_users, k, exclude_seen)


# the small model the CPU and the GPU test share: 300 users x 120 Zipf items, 4000 events with repeats, rank 8
SMALL = {"rank": 8, "reg": 0.01, "alpha": 40.0, "weighted_reg": False}
SMALL_HALF_SWEEPS = 6


def small_events(seed=4):
    """(user ids, item ids) of the small model: sparse id spaces, so that positions and ids differ."""
    u, i = zipf_events(np.random.default_rng(seed), 300, 120, 4000)
    return u * 3 + 1, i * 2 + 5


def initial_items(ni, rank, seed=0, scale=None):
    """The item factors ImplicitALS starts from: the seeded CPU generator of torch, scaled by rank^-1/2."""
    import torch
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(ni, rank, generator=gen) * (float(rank) ** -0.5 if scale is None else scale)).numpy()

"""Exactly representable ALS problems and their oracle, shared by test_gpu_als_exact.py and test_gpu_als_scale.py.

Factor entries are integers in [-2, 2], explicit targets are half-stars (0.5 .. 5.0), implicit weights are 0.5 x [1, 40].
Every product y_i y_j, d y_i, fl32(w y_i) y_j and c y_i (c = 1 + w) is then a multiple of 1/2, and as long as the sum of
their ABSOLUTE values over a row stays below 2^23 halves every partial sum, in any order and with any rounding inside the
matrix instruction, is exact in float32 (``assert_exact`` checks that on the host).  The Gram matrix, the right-hand side,
the whole-table G and the chunk sums are therefore the exact dyadics computed here in int64, and what follows them is IEEE
float32 alone: lam = fl32(reg n), the diagonal add, fmaf, a correctly rounded square root and division.  So a kernel row
must equal ``_als_ref.cholesky_solve32`` on ``_als_ref.fma32_exact`` in every bit."""
import numpy as np

import _als_ref as ref
from _als_ref import F32

N_OTHER = 97
LIMIT = 2 ** 23          # in halves: every partial and total below it is exact in float32


def table(rank, seed=0, n=N_OTHER):
    """float32 [n, rank] of integers in [-2, 2]."""
    return np.random.default_rng(7000 + 100 * seed + rank).integers(-2, 3, (n, rank)).astype(F32)


def values(rng, n, implicit):
    """Explicit: half-star targets 0.5 .. 5.0; implicit: weights 0.5 x [1, 40]."""
    return (rng.integers(1, 41 if implicit else 11, n) * 0.5).astype(F32)


def make_rows(rng, lens, implicit, n_other=N_OTHER, special=()):
    """(offsets int64, cols int32, values float32) of random rows of the lengths `lens` followed by the rows of explicit
    column lists `special`."""
    rows = [rng.integers(0, n_other, n) for n in lens] + [np.asarray(s, np.int64) for s in special]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return offsets, cols, values(rng, len(cols), implicit)


def halves(v):
    h = np.rint(np.asarray(v, np.float64) * 2).astype(np.int64)
    assert np.array_equal(h * 0.5, np.asarray(v, np.float64)), "not a multiple of 1/2"
    return h


def int_table(Y):
    t = np.rint(Y).astype(np.int64)
    assert np.array_equal(t.astype(F32), Y), "not an integer table"
    return t


def exact_sums(Y, cols, v, implicit, G=None):
    """One row's exact system before lam, and the largest sum of absolute values in halves: (A float32 [rank, rank],
    b float32 [rank], bound).  Explicit: A = sum y y^T, b = sum d y.  Implicit: A = G + sum w y y^T, b = sum (1 + w) y."""
    y = int_table(Y)[np.asarray(cols, np.int64)]
    h = halves(v)
    if implicit:
        A2, b2 = (y * h[:, None]).T @ y + 2 * int_table(G), y.T @ (2 + h)
        bound = max(((np.abs(y) * h[:, None]).T @ np.abs(y)).max() + 2 * np.abs(G).max(), (np.abs(y).T @ (2 + h)).max())
    else:
        A2, b2 = 2 * (y.T @ y), y.T @ h
        bound = max(2 * (np.abs(y).T @ np.abs(y)).max(), (np.abs(y).T @ np.abs(h)).max())
    return (A2 * 0.5).astype(F32), (b2 * 0.5).astype(F32), int(bound)


def int_gram(Y):
    """The exact integer Gram matrix of an integer table, and the largest sum of squares of one column."""
    t = int_table(Y)
    G = t.T @ t
    return G, int(np.diag(G).max()) if len(t) else 0


def oracle_rows(Y, offsets, cols, v, reg, weighted, implicit, fill, G=None):
    """(float32 [n_rows, rank], failures, largest bound): per row the Cholesky and the two solves of the kernel's contract on
    the exact system, on the correctly rounded fma; zeros for an empty row; `fill` where the contract refuses the row (a
    pivot that is not finite and positive, a solution that is not finite)."""
    n_rows, rank = len(offsets) - 1, Y.shape[1]
    out = np.full((n_rows, rank), fill, F32)
    failures = worst = 0
    for r in range(n_rows):
        a, e = int(offsets[r]), int(offsets[r + 1])
        if e == a:
            out[r] = 0
            continue
        A, b, bound = exact_sums(Y, cols[a:e], v[a:e], implicit, G)
        worst = max(worst, bound)
        x = ref.cholesky_solve32(A, b, ref.lam32(reg, e - a, weighted), fma=ref.fma32_exact)
        if x is None or not np.all(np.isfinite(x)):
            failures += 1
        else:
            out[r] = x
    return out, failures, worst


def assert_exact(bound):
    assert 0 <= bound < LIMIT, "a partial sum can reach 2^23 halves: %d" % bound


def tile_rows(offsets, cols, v, which):
    """The CSR whose row r is a copy of the prototype row which[r] of (offsets, cols, v); no Python loop over rows."""
    which = np.asarray(which, np.int64)
    lens = np.diff(offsets)[which]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    src = np.repeat(offsets[:-1][which] - new_off[:-1], lens) + np.arange(new_off[-1], dtype=np.int64)
    return new_off, np.ascontiguousarray(cols[src]), np.ascontiguousarray(v[src])


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def solve(dev, Y, offsets, cols, v, reg, weighted, implicit, fill, a=None, b=None, out=None, gram_of=None):
    """One ops.als_solve_rows or ops.als_gram + ops.als_solve_rows_implicit call on host arrays: (out tensor, failure word).
    `gram_of`: the table whose Gram the implicit solve gets (default Y itself)."""
    import torch
    from esrecsys_amd import ops
    n_rows = len(offsets) - 1
    if out is None:
        out = torch.full((n_rows, Y.shape[1]), fill, dtype=torch.float32, device=dev)
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    other = torch.from_numpy(Y).to(dev)
    args = (np.ascontiguousarray(offsets, np.int64), torch.from_numpy(cols).to(dev), torch.from_numpy(v).to(dev),
            0 if a is None else a, n_rows if b is None else b, reg, weighted, out, failed)
    if implicit:
        gram = ops.als_gram(other if gram_of is None else torch.from_numpy(gram_of).to(dev))
        ops.als_solve_rows_implicit(other, gram, *args)
    else:
        ops.als_solve_rows(other, *args)
    return out, int(failed.item())

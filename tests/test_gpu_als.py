"""GPU: esr_als.hip and esrecsys_amd/factorization.py against the oracle of tests/_als_ref.py -- the row solve against fp64
within a bound measured from float32 itself, the order contract bit for bit, indices and failures, predict / residuals /
recommend bit-equal to the restatement, and the fit."""
import numpy as np
import pytest
import torch

import _als_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
ULP32 = 2.0 ** -23
N_OTHER = 97


def geometry():
    from esrecsys_amd import ops
    return ops.als_geometry()


def lengths():
    C, W = geometry()
    return [0, 1, 2, 3, C - 1, C, C + 1, 2 * C + 1, C * W - 1, C * W, C * W + 1, 3 * C * W + 5]


_problems, _grams = {}, {}


def problem(rank):
    """One CSR of the lengths above over N_OTHER columns: half-star targets, other-side factors N(0, 1 / rank).  Made once
    per rank and never changed."""
    if rank not in _problems:
        rng = np.random.default_rng(1000 + rank)
        lens = lengths()
        offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cols = rng.integers(0, N_OTHER, offsets[-1]).astype(np.int32)
        d = (rng.integers(-8, 9, offsets[-1]) * 0.5).astype(np.float32)
        Y = (rng.standard_normal((N_OTHER, rank)) / np.sqrt(rank)).astype(np.float32)
        _problems[rank] = (offsets, cols, d, Y)
    return _problems[rank]


def gram(rank, r):
    """The float32 restatement's Gram matrix and right-hand side of row r (they do not depend on reg): made once."""
    if (rank, r) not in _grams:
        offsets, cols, d, Y = problem(rank)
        a, e = int(offsets[r]), int(offsets[r + 1])
        _grams[(rank, r)] = ref.gram_rhs32(Y, cols[a:e], d[a:e], geometry()[0]) if e > a else None
    return _grams[(rank, r)]


def solve(dev, offsets, cols, d, Y, reg, weighted, a=None, b=None, out=None, fill=0.0):
    """ops.als_solve_rows on host arrays: (out tensor, failure word)."""
    from esrecsys_amd import ops
    n_rows = len(offsets) - 1
    if out is None:
        out = torch.full((n_rows, Y.shape[1]), fill, dtype=torch.float32, device=dev)
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.als_solve_rows(torch.from_numpy(Y).to(dev), np.ascontiguousarray(offsets, np.int64), torch.from_numpy(cols).to(dev),
                       torch.from_numpy(d).to(dev), 0 if a is None else a, n_rows if b is None else b, reg, weighted, out,
                       failed)
    return out, int(failed.item())


@pytest.mark.parametrize("reg", [0.1, 1e-3])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("rank", [1, 5, 32, 33, 64])
def test_row_solve_against_fp64(dev, rank, weighted, reg):
    offsets, cols, d, Y = problem(rank)
    out, word = solve(dev, offsets, cols, d, Y, reg, weighted, fill=7.0)
    assert word == 0
    got = out.cpu().numpy()
    for r in range(len(offsets) - 1):
        a, e = int(offsets[r]), int(offsets[r + 1])
        x64 = ref.solve_row64(Y, cols[a:e], d[a:e], reg, weighted)
        if e == a:
            assert np.array_equal(got[r], np.zeros(rank, np.float32))                  # no rating: the zero vector
            continue
        x32 = ref.solve_row32(Y, cols[a:e], d[a:e], reg, weighted, geometry()[0], gram=gram(rank, r))
        err_kernel, err_f32 = rel_err(got[r], x64), rel_err(x32, x64)
        print("rank %d weighted %d reg %g row %d (n = %d): kernel %.3e float32 restatement %.3e"
              % (rank, weighted, reg, r, e - a, err_kernel, err_f32))
        assert err_kernel <= 4 * err_f32 + 8 * ULP32, (r, e - a, err_kernel, err_f32)


@pytest.mark.parametrize("rank", [5, 64])
def test_order_contract_bit_for_bit(dev, rank):
    offsets, cols, d, Y = problem(rank)
    n_rows = len(offsets) - 1
    full, word = solve(dev, offsets, cols, d, Y, 0.1, True)
    again, _ = solve(dev, offsets, cols, d, Y, 0.1, True)
    assert word == 0 and torch.equal(full, again)
    pieces = torch.zeros_like(full)
    for a, b in ((0, 5), (5, 6), (6, 6), (6, 11), (11, n_rows)):
        solve(dev, offsets, cols, d, Y, 0.1, True, a, b, out=pieces)
    assert torch.equal(full, pieces)
    # the rows in another order in another CSR (each row's own ratings in order): the same bits per row
    perm = np.random.default_rng(2).permutation(n_rows)
    lens = np.diff(offsets)
    p_off = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64)
    p_cols = np.concatenate([cols[offsets[r]:offsets[r + 1]] for r in perm]).astype(np.int32)
    p_d = np.concatenate([d[offsets[r]:offsets[r + 1]] for r in perm]).astype(np.float32)
    permuted, _ = solve(dev, p_off, p_cols, p_d, Y, 0.1, True)
    assert torch.equal(permuted, full[torch.from_numpy(perm).to(dev)])


def small_model(dev, seed=4, **kw):
    from esrecsys_amd.factorization import RatingsALS
    u, i, r = ref.zipf_ratings(np.random.default_rng(seed), 300, 120, 4000)
    return RatingsALS(u * 3 + 1, i * 2 + 5, r, rank=8, reg=0.1, device=dev, **kw), (u * 3 + 1, i * 2 + 5, r)


def test_constructor_refusals_and_initialisation(dev):
    from esrecsys_amd.factorization import RatingsALS
    with pytest.raises(ValueError) as e:
        RatingsALS([3, 1, 3], [7, 7, 7], [4.0, 2.0, 1.5], rank=2, device=dev)
    assert str(e.value) == "a (user, item) is rated twice: keep one rating per pair (latest_ratings)"
    u, i, r = [3, 1, 3, 9], [7, 7, 2, 5], [4.0, 2.0, 1.5, 3.0]
    for scale, seed in ((None, 0), (0.5, 0), (2.0, 6)):
        m = RatingsALS(u, i, r, rank=3, seed=seed, init_scale=scale, device=dev)
        gen = torch.Generator(device="cpu").manual_seed(seed)
        want = torch.randn(3, 3, generator=gen) * (3 ** -0.5 if scale is None else scale)
        assert torch.equal(m.item_factors.cpu(), want) and not bool(m.user_factors.any())
        assert m.users.tolist() == [1, 3, 9] and m.items.tolist() == [2, 5, 7]
        assert m.users.dtype == m.items.dtype == torch.int32 and m.user_mean.tolist() == [2.0, 2.75, 3.0]
    # a query id that does not fit int32 is unknown, never wrapped onto a known one
    m.sweep()
    big = np.array([3, 3 + 2 ** 32, 2 ** 31 + 1, -1], np.int64)
    p = m.predict(big, np.full(4, 7, np.int64)).cpu().numpy()
    assert not np.isnan(p[0]) and np.all(np.isnan(p[1:]))
    p = m.predict(np.full(4, 3, np.int64), big + 4).cpu().numpy()          # item 7, then ids outside int32
    assert not np.isnan(p[0]) and np.all(np.isnan(p[1:]))
    ids, sc, ln = m.recommend(big, k=2, exclude_rated=False)
    assert ln.tolist() == [2, 0, 0, 0]


def test_max_rows_per_launch_does_not_change_a_bit(dev):
    base, _ = small_model(dev)
    base.sweep()
    for cut in (1, 7):
        m, _ = small_model(dev, max_rows_per_launch=cut)
        m.sweep()
        assert torch.equal(m.user_factors, base.user_factors) and torch.equal(m.item_factors, base.item_factors)


def test_indices_and_failures(dev):
    from esrecsys_amd.factorization import FactorizationError, RatingsALS
    rank = 5
    rng = np.random.default_rng(8)
    Y = (rng.standard_normal((N_OTHER, rank)) / np.sqrt(rank)).astype(np.float32)
    # rows: the first and the last position; all ratings on one column; an ordinary row
    rows = [[0, N_OTHER - 1], [13] * 9, list(rng.integers(0, N_OTHER, 6))]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.concatenate(rows).astype(np.int32)
    d = (rng.integers(-8, 9, len(cols)) * 0.5).astype(np.float32)
    out, word = solve(dev, offsets, cols, d, Y, 0.1, True)
    assert word == 0
    want = ref.half_sweep(Y, offsets, cols, d, 0.1, True)
    f32 = ref.half_sweep(Y, offsets, cols, d, 0.1, True, chunk=geometry()[0])
    assert rel_err(out.cpu().numpy(), want) <= 4 * rel_err(f32, want) + 8 * ULP32
    for bad in (-1, N_OTHER, 2 ** 31 - 1):       # never dereferenced; the other rows are still correct
        c2 = cols.copy()
        c2[3] = bad
        out2, word2 = solve(dev, offsets, c2, d, Y, 0.1, True)
        assert word2 & (1 << 30)
        assert torch.equal(out2[0], out[0]) and torch.equal(out2[2], out[2])
    # a NaN factor row: the rows that read it fail and stay as they were, the others are solved
    Yn = Y.copy()
    Yn[13, 2] = np.nan
    out3, word3 = solve(dev, offsets, cols, d, Yn, 0.1, True, fill=7.0)
    touched = [13 in r for r in rows]
    assert word3 == sum(touched)
    for r, t in enumerate(touched):
        assert torch.equal(out3[r], torch.full_like(out3[r], 7.0) if t else out[r])
    # the module turns both into exceptions after the launch
    m = RatingsALS([0, 0, 1, 2], [0, 1, 1, 0], [3.0, 4.0, 2.5, 5.0], rank=2, device=dev)
    before = m.user_factors.clone()
    m.item_factors[1, 0] = float("nan")
    with pytest.raises(FactorizationError, match="2 row"):
        m.solve_users()
    assert torch.equal(m.user_factors[[0, 1]], before[[0, 1]]) and bool(torch.isfinite(m.user_factors).all())
    m._row_ipos[0] = 9
    with pytest.raises(FactorizationError, match="position"):
        m.solve_users()


@pytest.mark.parametrize("center", ["user", "global", "none"])
@pytest.mark.parametrize("rank", [1, 5, 64])
def test_predict_and_residuals_equal_the_oracle_bits(dev, rank, center):
    from esrecsys_amd.factorization import RatingsALS
    rng = np.random.default_rng(rank)
    u, i, r = ref.zipf_ratings(rng, 40, 30, 300)
    m = RatingsALS(u * 2, i * 3, r, rank=rank, center=center, device=dev)
    m.user_factors.copy_(torch.from_numpy(rng.standard_normal((m.users.numel(), rank)).astype(np.float32)))
    X, Y = m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy()
    users, items, c = m.users.cpu().numpy(), m.items.cpu().numpy(), m.user_mean.cpu().numpy()
    if center == "global":
        assert np.all(c == np.float64(np.sum(r, dtype=np.float64) / len(r)))
    if center == "none":
        assert np.all(c == 0)
    for nq in (0, 1, 257):
        qu = rng.choice(np.concatenate([users, [1, 10 ** 6]]), nq)        # odd ids and 10^6 are unknown
        qi = rng.choice(np.concatenate([items, [1, 10 ** 6]]), nq)
        upos = np.array([np.searchsorted(users, x) if x in users else -1 for x in qu], np.int64)
        ipos = np.array([np.searchsorted(items, x) if x in items else -1 for x in qi], np.int64)
        got = m.predict(qu, qi).cpu().numpy()
        want = ref.predict(X, Y, upos, ipos, c)
        assert got.dtype == np.float32 and got.shape == (nq,)
        assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
        assert np.array_equal(np.isnan(got), np.isnan(want)) and (nq < 257 or np.isnan(want).any())
    res = m.residuals().cpu().numpy()
    want = ref.residuals(X, Y, m._row_upos.cpu().numpy(), m._row_ipos.cpu().numpy(), m._targets.cpu().numpy())
    assert np.array_equal(res.view(np.uint32), want.view(np.uint32))
    # the targets: float32(float64(r) - c[u]) in CSR-by-user order
    order = np.lexsort((i, u))
    assert np.array_equal(m._targets.cpu().numpy(), (r[order] - c[np.searchsorted(users, u[order] * 2)]).astype(np.float32))


def test_fit(dev):
    m, (u, i, r) = small_model(dev)
    Y0 = m.item_factors.cpu().numpy().copy()
    gen = torch.Generator(device="cpu").manual_seed(0)
    assert np.array_equal(Y0, (torch.randn(m.items.numel(), 8, generator=gen) * 8 ** -0.5).numpy())
    assert not bool(m.user_factors.any())
    history = m.fit(sweeps=3)
    assert len(history) == 6 and all(isinstance(h, float) for h in history)
    upos, ipos, d = m._row_upos.cpu().numpy(), m._row_ipos.cpu().numpy(), m._targets.cpu().numpy()
    X, Y = m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy()
    want = ref.objective(X, Y, upos, ipos, d, 0.1, True)
    assert abs(history[-1] - want) <= 1e-12 * want and abs(m.objective() - want) <= 1e-12 * want
    # non-increasing up to the float32 restatement's own wobble (expected: none)
    _, _, h32 = ref.fit(upos, ipos, d, Y0, 0.1, True, 6, chunk=geometry()[0])
    wobble = max([0.0] + [(b - a) / a for a, b in zip(h32, h32[1:])])
    print("objective: kernel %s restatement %s (largest relative increase %.3e)" % (history, h32, wobble))
    for a, b in zip(history, history[1:]):
        assert b <= a * (1 + 4 * wobble), history
    m2, _ = small_model(dev)
    m2.fit(sweeps=3)
    assert torch.equal(m2.user_factors, m.user_factors) and torch.equal(m2.item_factors, m.item_factors)
    pred = m.predict(u, i).cpu().numpy().astype(np.float64)
    assert abs(m.rmse(u, i, r) - np.sqrt(np.mean((pred - r) ** 2))) <= 1e-12
    assert np.isnan(m.rmse([2], [4], [1.0]))                                   # an unknown user: no pair to score


def rated_sets(u, i):
    out = {}
    for a, b in zip(u.tolist(), i.tolist()):
        out.setdefault(a, set()).add(b)
    return out


def test_recommend_whole_corpus_equals_the_oracle(dev):
    from esrecsys_amd import evaluate
    m, (u, i, r) = small_model(dev)
    m.fit(sweeps=1)
    X, Y, c = m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy(), m.user_mean.cpu().numpy()
    users, items = m.users.cpu().numpy(), m.items.cpu().numpy()
    # a user who rated everything, an unknown one (id 0), the rest
    everything = RatedAll(dev, items)
    queries = np.concatenate([users[:40], [0]])
    for exclude in (True, False):
        ids, sc, ln = m.recommend(queries, k=110, exclude_rated=exclude, slack=16)        # k' = ni = 120
        w_ids, w_sc, w_ln = ref.recommend(X, Y, c, users, items, rated_sets(u, i), queries, 110, exclude)
        assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and ln.dtype == torch.int32
        assert np.array_equal(ln.cpu().numpy(), w_ln) and np.array_equal(ids.cpu().numpy(), w_ids)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), w_sc.view(np.uint32))
        assert int(ln[-1]) == 0
    ids, sc, ln = everything.recommend([7], k=10)
    assert int(ln[0]) == 0 and bool((ids == -1).all()) and bool((sc == 0).all())
    ids, sc, ln = m.recommend(queries, k=10)
    truth = torch.arange(len(queries), dtype=torch.int32) % 3 + 5
    metrics = evaluate.ranking_metrics(ids, ln, truth, np.arange(len(queries) + 1, dtype=np.int64), ks=(1, 10))
    assert metrics.mean()["n_valid"] >= 1


def RatedAll(dev, items):
    from esrecsys_amd.factorization import RatingsALS
    ni = len(items)
    m = RatingsALS(np.concatenate([np.full(ni, 7), [8]]), np.concatenate([items, items[:1]]),
                   np.concatenate([np.full(ni, 3.5), [2.0]]), rank=4, device=dev)
    m.sweep()
    return m


BIG_SEED = 29    # checked on the CPU (seeds 0..29 tried; the smallest gap is 1.8e-4 x the largest score): with this seed the oracle's gap between ranks k and k + 1 exceeds 1e-4 x the largest
                 # score for every query below (the test asserts it again)
BIG_ITEMS = 5000


def big_problem(seed):
    """6000 Zipf ratings of users 0..399 over BIG_ITEMS item ids, and one rating of EVERY item by the users 1000..1099 (50
    items each: none of them is queried), so that the model holds all BIG_ITEMS items; factors drawn from the seed."""
    rng = np.random.default_rng(seed)
    u, i, r = ref.zipf_ratings(rng, 400, BIG_ITEMS, 6000)
    every = np.arange(BIG_ITEMS, dtype=np.int64)
    u = np.concatenate([u, 1000 + every // 50])
    i = np.concatenate([i, every])
    r = np.concatenate([r, rng.integers(1, 11, BIG_ITEMS) * 0.5])
    X = (rng.standard_normal((len(np.unique(u)), 16)) * 0.25).astype(np.float32)
    Y = (rng.standard_normal((BIG_ITEMS, 16)) * 0.25).astype(np.float32)
    return u, i, r, X, Y, np.unique(u)[:16]


def gaps_ok(X, Y, c, users, items, rated, queries, k):
    ids, sc, ln = ref.recommend(X, Y, c, users, items, rated, queries, k + 1)
    assert np.all(ln == k + 1)
    return np.all(sc[:, k - 1].astype(np.float64) - sc[:, k] > 1e-4 * np.max(np.abs(sc), axis=1)), (ids[:, :k], sc[:, :k])


def test_recommend_large_corpus(dev):
    from esrecsys_amd.factorization import RatingsALS
    k = 50
    u, i, r, X, Y, queries = big_problem(BIG_SEED)
    m = RatingsALS(u, i, r, rank=16, device=dev)
    users, items = m.users.cpu().numpy(), m.items.cpu().numpy()
    assert m.items.numel() == BIG_ITEMS == 5000 and len(users) == len(X) and np.all(queries < 400)
    m.user_factors.copy_(torch.from_numpy(X))
    m.item_factors.copy_(torch.from_numpy(Y))
    c = m.user_mean.cpu().numpy()
    rated = rated_sets(u, i)
    ok, (w_ids, w_sc) = gaps_ok(X, Y, c, users, items, rated, queries, k)
    assert ok, "BIG_SEED no longer separates ranks k and k + 1"
    ids, sc, ln = (t.cpu().numpy() for t in m.recommend(queries, k=k))
    assert np.all(ln == k)
    flat_u = np.repeat(queries, k)
    assert np.array_equal(sc.reshape(-1).view(np.uint32), m.predict(flat_u, ids.reshape(-1)).cpu().numpy().view(np.uint32))
    for q, user in enumerate(queries):
        assert not rated[int(user)] & set(ids[q].tolist())
        key = list(zip((-sc[q].astype(np.float64)).tolist(), ids[q].tolist()))
        assert key == sorted(key)
        assert set(ids[q].tolist()) == set(w_ids[q].tolist()), q
    assert np.array_equal(ids, w_ids) and np.array_equal(sc.view(np.uint32), w_sc.view(np.uint32))
    # k' above what retrieve_topk selects: refused, the query named
    with pytest.raises(ValueError, match="query"):
        m.recommend(queries, k=1000, slack=16)
    with pytest.raises(ValueError, match="query"):
        m.recommend(queries, k=1020, exclude_rated=False, slack=16)

"""GPU: the implicit-feedback ALS of esr_als.hip and esrecsys_amd/factorization.py (ImplicitALS) against the oracle of
tests/_ials_ref.py -- the whole-table Gram and the row solve against fp64 within a bound measured from float32 itself, the
order contract bit for bit, indices, weights and failures, and the model: fit, objective, score, recommend, fold-in."""
import numpy as np
import pytest
import torch

import _als_ref as ref
import _ials_ref as iref
from conftest import rel_err

pytestmark = pytest.mark.gpu
ULP32 = 2.0 ** -23
N_OTHER = 97


def geometry():
    from esrecsys_amd import ops
    return ops.als_geometry()


def segment():
    from esrecsys_amd import ops
    return ops.als_gram_geometry()


def lengths():
    C, W = geometry()
    return [0, 1, 2, 3, C - 1, C, C + 1, 2 * C + 1, C * W - 1, C * W, C * W + 1, 3 * C * W + 5]


# ---- the whole-table Gram ---------------------------------------------------------------------------------------------------
_tables = {}


def table(rank):
    """2 S + 3 rows N(0, 1 / rank), made once per rank and never changed; the cases take its leading rows."""
    if rank not in _tables:
        _tables[rank] = (np.random.default_rng(500 + rank).standard_normal((2 * segment() + 3, rank))
                         / np.sqrt(rank)).astype(np.float32)
    return _tables[rank]


def gram_sizes():
    S = segment()
    return [0, 1, 2, 63, 65, S - 1, S, S + 1, 2 * S + 3]


@pytest.mark.parametrize("case", range(9))
@pytest.mark.parametrize("rank", [1, 5, 32, 33, 64])
def test_gram_against_fp64(dev, rank, case):
    from esrecsys_amd import ops
    S, n = segment(), gram_sizes()[case]
    Y = table(rank)[:n]
    t = torch.from_numpy(Y).to(dev)
    got_t = ops.als_gram(t)
    got = got_t.cpu().numpy()
    assert got.shape == (rank, rank) and got.dtype == np.float32
    g64, g32 = iref.gram64(Y), iref.gram32(Y, S)
    err_kernel, err_f32 = rel_err(got, g64), rel_err(g32, g64)
    print("gram rank %d n %d: kernel %.3e float32 restatement %.3e" % (rank, n, err_kernel, err_f32))
    assert err_kernel <= 4 * err_f32 + 8 * ULP32, (rank, n, err_kernel, err_f32)
    assert np.array_equal(got.view(np.uint32), got.T.view(np.uint32))                       # exactly symmetric
    if n == 0:
        assert not got.any()
    assert torch.equal(ops.als_gram(t), got_t)                                                # a repeat: the same bits
    for extra in (1, S, S + 1):                                                               # trailing all-zero rows
        longer = torch.cat([t, torch.zeros((extra, rank), dtype=torch.float32, device=dev)])
        assert torch.equal(ops.als_gram(longer), got_t), extra
    out = torch.full((rank, rank), 7.0, dtype=torch.float32, device=dev)
    assert ops.als_gram(t, out=out) is out and torch.equal(out, got_t)


# ---- the row solve ------------------------------------------------------------------------------------------------------------
_problems, _partials = {}, {}


def problem(rank):
    """One CSR of the lengths above over N_OTHER columns: weights 0.5 * integers in [1, 40], other-side factors
    N(0, 1 / rank), their Gram in fp64 and in the float32 restatement.  Made once per rank and never changed."""
    if rank not in _problems:
        rng = np.random.default_rng(2000 + rank)
        offsets = np.concatenate([[0], np.cumsum(lengths())]).astype(np.int64)
        cols = rng.integers(0, N_OTHER, offsets[-1]).astype(np.int32)
        w = (rng.integers(1, 41, offsets[-1]) * 0.5).astype(np.float32)
        Y = (rng.standard_normal((N_OTHER, rank)) / np.sqrt(rank)).astype(np.float32)
        _problems[rank] = (offsets, cols, w, Y, iref.gram64(Y), iref.gram32(Y, segment()))
    return _problems[rank]


def partial(rank, r):
    """The float32 restatement's weighted Gram and right-hand side of row r (they do not depend on reg): made once."""
    if (rank, r) not in _partials:
        offsets, cols, w, Y, _, _ = problem(rank)
        a, e = int(offsets[r]), int(offsets[r + 1])
        _partials[(rank, r)] = iref.gram_rhs32(Y, cols[a:e], w[a:e], geometry()[0]) if e > a else None
    return _partials[(rank, r)]


def solve(dev, offsets, cols, w, Y, reg, weighted, a=None, b=None, out=None, fill=0.0):
    """ops.als_gram + ops.als_solve_rows_implicit on host arrays: (out tensor, failure word)."""
    from esrecsys_amd import ops
    n_rows = len(offsets) - 1
    if out is None:
        out = torch.full((n_rows, Y.shape[1]), fill, dtype=torch.float32, device=dev)
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    other = torch.from_numpy(Y).to(dev)
    ops.als_solve_rows_implicit(other, ops.als_gram(other), np.ascontiguousarray(offsets, np.int64),
                                torch.from_numpy(cols).to(dev), torch.from_numpy(w).to(dev), 0 if a is None else a,
                                n_rows if b is None else b, reg, weighted, out, failed)
    return out, int(failed.item())


@pytest.mark.parametrize("reg", [0.1, 1e-3])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("rank", [1, 5, 32, 33, 64])
def test_row_solve_against_fp64(dev, rank, weighted, reg):
    offsets, cols, w, Y, g64, g32 = problem(rank)
    out, word = solve(dev, offsets, cols, w, Y, reg, weighted, fill=7.0)
    assert word == 0
    got = out.cpu().numpy()
    for r in range(len(offsets) - 1):
        a, e = int(offsets[r]), int(offsets[r + 1])
        if e == a:
            assert np.array_equal(got[r], np.zeros(rank, np.float32))                  # no entry: the zero vector
            continue
        x64 = iref.solve_row64(Y, cols[a:e], w[a:e], g64, reg, weighted)
        x32 = iref.solve_row32(Y, cols[a:e], w[a:e], g32, reg, weighted, geometry()[0], partial=partial(rank, r))
        err_kernel, err_f32 = rel_err(got[r], x64), rel_err(x32, x64)
        print("rank %d weighted %d reg %g row %d (n = %d): kernel %.3e float32 restatement %.3e"
              % (rank, weighted, reg, r, e - a, err_kernel, err_f32))
        assert err_kernel <= 4 * err_f32 + 8 * ULP32, (r, e - a, err_kernel, err_f32)


@pytest.mark.parametrize("rank", [5, 64])
def test_order_contract_bit_for_bit(dev, rank):
    offsets, cols, w, Y, _, _ = problem(rank)
    n_rows = len(offsets) - 1
    full, word = solve(dev, offsets, cols, w, Y, 0.1, True)
    again, _ = solve(dev, offsets, cols, w, Y, 0.1, True)
    assert word == 0 and torch.equal(full, again)
    pieces = torch.zeros_like(full)
    for a, b in ((0, 5), (5, 6), (6, 6), (6, 11), (11, n_rows)):
        solve(dev, offsets, cols, w, Y, 0.1, True, a, b, out=pieces)
    assert torch.equal(full, pieces)
    # the rows in another order in another CSR (each row's own entries in order): the same bits per row
    perm = np.random.default_rng(2).permutation(n_rows)
    lens = np.diff(offsets)
    p_off = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64)
    p_cols = np.concatenate([cols[offsets[r]:offsets[r + 1]] for r in perm]).astype(np.int32)
    p_w = np.concatenate([w[offsets[r]:offsets[r + 1]] for r in perm]).astype(np.float32)
    permuted, _ = solve(dev, p_off, p_cols, p_w, Y, 0.1, True)
    assert torch.equal(permuted, full[torch.from_numpy(perm).to(dev)])


def test_indices_weights_and_failures(dev):
    from esrecsys_amd.factorization import FactorizationError, ImplicitALS
    rank = 5
    rng = np.random.default_rng(8)
    Y = (rng.standard_normal((N_OTHER, rank)) / np.sqrt(rank)).astype(np.float32)
    # rows: the first and the last position; all entries on one column; an ordinary row
    rows = [[0, N_OTHER - 1], [13] * 9, list(rng.integers(0, N_OTHER, 6))]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = np.concatenate(rows).astype(np.int32)
    w = (rng.integers(1, 41, len(cols)) * 0.5).astype(np.float32)
    out, word = solve(dev, offsets, cols, w, Y, 0.1, False)
    assert word == 0
    want = iref.half_sweep(Y, offsets, cols, w, 0.1, False)
    f32 = iref.half_sweep(Y, offsets, cols, w, 0.1, False, chunk=geometry()[0], segment=segment())
    assert rel_err(out.cpu().numpy(), want) <= 4 * rel_err(f32, want) + 8 * ULP32
    # the ordinary row with ONE more entry at its end that does not count: the rest of the row is still used, bit for bit
    # (lam does not depend on the count without weighted)
    off2 = offsets.copy()
    off2[-1] += 1
    for col, weight, bit in ((-1, 1.0, 30), (N_OTHER, 1.0, 30), (2 ** 31 - 1, 1.0, 30), (3, -0.5, 29), (3, np.nan, 29),
                             (3, np.inf, 29), (3, -np.inf, 29)):
        out2, word2 = solve(dev, off2, np.append(cols, np.int32(col)), np.append(w, np.float32(weight)), Y, 0.1, False)
        assert word2 == 1 << bit, (col, weight, word2)
        assert torch.equal(out2, out), (col, weight)
    out2, word2 = solve(dev, off2, np.append(cols, np.int32(-7)), np.append(w, np.float32(np.nan)), Y, 0.1, False)
    assert word2 == (1 << 30) | (1 << 29) and torch.equal(out2, out)
    out2, word2 = solve(dev, off2, np.append(cols, np.int32(3)), np.append(w, np.float32(0.0)), Y, 0.1, False)
    assert word2 == 0 and not torch.equal(out2[2], out[2])                       # weight 0: a seen cell at confidence 1
    # a NaN factor row: the Gram is NaN, every row with entries fails and stays as it was
    Yn = Y.copy()
    Yn[13, 2] = np.nan
    out3, word3 = solve(dev, offsets, cols, w, Yn, 0.1, False, fill=7.0)
    assert word3 == 3 and bool((out3 == 7.0).all())
    # ... and with a finite Gram only the rows that read it
    from esrecsys_amd import ops
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    out4 = torch.full((3, rank), 7.0, dtype=torch.float32, device=dev)
    ops.als_solve_rows_implicit(torch.from_numpy(Yn).to(dev), ops.als_gram(torch.from_numpy(Y).to(dev)), offsets,
                                torch.from_numpy(cols).to(dev), torch.from_numpy(w).to(dev), 0, 3, 0.1, False, out4, failed)
    touched = [13 in r for r in rows]
    assert int(failed.item()) == sum(touched)
    for r, t in enumerate(touched):
        assert torch.equal(out4[r], torch.full_like(out4[r], 7.0) if t else out[r])
    # the module turns the words into exceptions after the launch
    m = ImplicitALS([0, 0, 1, 2], [0, 1, 1, 0], rank=2, device=dev)
    before = m.user_factors.clone()
    m.item_factors[1, 0] = float("nan")
    with pytest.raises(FactorizationError, match="3 row"):
        m.solve_users()
    assert torch.equal(m.user_factors, before)
    m = ImplicitALS([0, 0, 1, 2], [0, 1, 1, 0], rank=2, device=dev)
    m._weights[1] = -1.0
    with pytest.raises(FactorizationError, match="weight"):
        m.solve_users()
    m._weights[1] = 1.0
    m._row_ipos[0] = 9
    with pytest.raises(FactorizationError, match="position"):
        m.solve_users()


# ---- the model ------------------------------------------------------------------------------------------------------------------
def small_model(dev, **kw):
    from esrecsys_amd.factorization import ImplicitALS
    user, item = iref.small_events()
    return ImplicitALS(user, item, device=dev, **dict(iref.SMALL, **kw)), (user, item)


def pairs_of(m):
    return m._row_upos.cpu().numpy().astype(np.int64), m._row_ipos.cpu().numpy().astype(np.int64), m._weights.cpu().numpy()


def seen_sets(u, i):
    out = {}
    for a, b in zip(u.tolist(), i.tolist()):
        out.setdefault(a, set()).add(b)
    return out


def test_constructor_refusals_and_initialisation(dev):
    from esrecsys_amd.factorization import ImplicitALS
    u, i, s = [3, 1, 3, 9, 3], [7, 7, 2, 5, 7], [1.0, 2.0, 0.5, 3.0, 0.25]
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            ImplicitALS(u, i, s, rank=2, alpha=alpha, device=dev)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            ImplicitALS(u, i, [1.0, bad, 0.5, 3.0, 0.25], rank=2, device=dev)
    with pytest.raises(ValueError, match="ids"):
        ImplicitALS([-1, 2], [0, 1], rank=2, device=dev)
    with pytest.raises(ValueError, match="rank"):
        ImplicitALS(u, i, s, rank=65, device=dev)
    with pytest.raises(ValueError, match="reg"):
        ImplicitALS(u, i, s, rank=2, reg=0.0, device=dev)
    for scale, seed in ((None, 0), (0.5, 0), (2.0, 6)):
        m = ImplicitALS(u, i, s, rank=3, alpha=4.0, seed=seed, init_scale=scale, device=dev)
        assert torch.equal(m.item_factors.cpu(), torch.from_numpy(iref.initial_items(3, 3, seed, scale)))
        assert not bool(m.user_factors.any())
        assert m.users.tolist() == [1, 3, 9] and m.items.tolist() == [2, 5, 7]
        # repeated events add their strengths: (3, 7) was seen twice
        assert m._row_upos.tolist() == [0, 1, 1, 2] and m._row_ipos.tolist() == [2, 0, 2, 1]
        assert m._weights.tolist() == [8.0, 2.0, 5.0, 12.0] and m.nnz == 4
    m = ImplicitALS(u, i, rank=3, device=dev)                                     # no strength: every event counts 1
    assert m._weights.tolist() == [40.0, 40.0, 80.0, 40.0]
    d = ImplicitALS.from_documents([7, 2, 7, 7, 5], [0, 3, 3, 5], rank=3, alpha=2.0, device=dev)
    assert d.users.tolist() == [0, 2] and d.items.tolist() == [2, 5, 7]
    assert d._row_ipos.tolist() == [0, 2, 1, 2] and d._weights.tolist() == [2.0, 4.0, 2.0, 2.0]


def test_max_rows_per_launch_does_not_change_a_bit(dev):
    base, _ = small_model(dev)
    base.sweep()
    for cut in (1, 7):
        m, _ = small_model(dev, max_rows_per_launch=cut)
        m.sweep()
        assert torch.equal(m.user_factors, base.user_factors) and torch.equal(m.item_factors, base.item_factors)


def test_fit_objective_and_score(dev):
    m, (user, item) = small_model(dev)
    assert np.array_equal(m.item_factors.cpu().numpy(), iref.initial_items(m.items.numel(), 8))
    history = m.fit(sweeps=iref.SMALL_HALF_SWEEPS // 2)
    assert len(history) == iref.SMALL_HALF_SWEEPS and all(isinstance(h, float) for h in history)
    print("objective after every half-sweep: %s" % (history,))
    for a, b in zip(history, history[1:]):
        assert b <= a * (1 + 1e-6), history
    u, i, w = pairs_of(m)
    X, Y = m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy()
    want = iref.objective_dense(X, Y, u, i, w, iref.SMALL["reg"], iref.SMALL["weighted_reg"])
    print("objective: module %.17g dense oracle %.17g" % (m.objective(), want))
    assert abs(m.objective() - want) <= 1e-9 * want and abs(history[-1] - want) <= 1e-9 * want
    m2, _ = small_model(dev)
    m2.fit(sweeps=iref.SMALL_HALF_SWEEPS // 2)
    assert torch.equal(m2.user_factors, m.user_factors) and torch.equal(m2.item_factors, m.item_factors)
    # the training pairs are the oracle's
    users, items = m.users.cpu().numpy().astype(np.int64), m.items.cpu().numpy().astype(np.int64)
    ou, oi, ow = iref.sum_events(np.searchsorted(users, user), np.searchsorted(items, item), None, iref.SMALL["alpha"])
    assert np.array_equal(ou, u) and np.array_equal(oi, i) and np.array_equal(ow, w)
    # score: the oracle's predict without an offset, bit for bit; NaN for unknown ids
    rng = np.random.default_rng(3)
    qu = rng.choice(np.concatenate([users, [0, 10 ** 6]]), 257)
    qi = rng.choice(np.concatenate([items, [0, 10 ** 6]]), 257)
    upos = np.array([np.searchsorted(users, x) if x in users else -1 for x in qu], np.int64)
    ipos = np.array([np.searchsorted(items, x) if x in items else -1 for x in qi], np.int64)
    got, exp = m.score(qu, qi).cpu().numpy(), ref.predict(X, Y, upos, ipos)
    assert np.isnan(exp).any() and np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(got.view(np.uint32)[~np.isnan(exp)], exp.view(np.uint32)[~np.isnan(exp)])
    with pytest.raises(ValueError, match="one length"):
        m.score(qu, qi[:5])


def test_weighted_reg_objective(dev):
    m, _ = small_model(dev, weighted_reg=True, reg=0.05)
    history = m.fit(sweeps=1)
    u, i, w = pairs_of(m)
    want = iref.objective_dense(m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy(), u, i, w, 0.05, True)
    assert abs(history[-1] - want) <= 1e-9 * want and history[1] <= history[0] * (1 + 1e-6)


def test_recommend_equals_the_full_sort_oracle(dev):
    m, (user, item) = small_model(dev)
    m.fit(sweeps=1)
    X, Y = m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy()
    users, items = m.users.cpu().numpy(), m.items.cpu().numpy()
    queries = np.concatenate([users[:40], [0]])                                   # id 0 is unknown
    k = m.items.numel() - 10
    for exclude in (True, False):
        ids, sc, ln = m.recommend(queries, k=k, exclude_seen=exclude, slack=16)   # k' = ni: every item is a candidate
        w_ids, w_sc, w_ln = iref.recommend(X, Y, users, items, seen_sets(user, item), queries, k, exclude)
        assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and ln.dtype == torch.int32
        assert np.array_equal(ln.cpu().numpy(), w_ln) and np.array_equal(ids.cpu().numpy(), w_ids)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), w_sc.view(np.uint32))
        assert int(ln[-1]) == 0
    ids, sc, ln = (t.cpu().numpy() for t in m.recommend(queries[:8], k=5))
    flat = m.score(np.repeat(queries[:8], 5), ids.reshape(-1)).cpu().numpy()
    assert np.array_equal(sc.reshape(-1).view(np.uint32), flat.view(np.uint32))
    with pytest.raises(ValueError, match="k ="):
        m.recommend(queries, k=0)
    with pytest.raises(ValueError, match="slack"):
        m.recommend(queries, k=5, slack=-1)


def test_fold_in_and_recommend_documents(dev):
    from esrecsys_amd import evaluate
    m, (user, item) = small_model(dev)
    m.fit(sweeps=1)
    m.solve_users()                                                                # the user rows of the CURRENT item factors
    users, items = m.users.cpu().numpy(), m.items.cpu().numpy()
    Y = m.item_factors.cpu().numpy()
    # every training user's own events as a document (repeats and all, in the events' order): that user's row, bit for bit
    order = np.argsort(user, kind="stable")
    doc_off = np.concatenate([[0], np.cumsum(np.bincount(np.searchsorted(users, user)))]).astype(np.int64)
    own = m.fold_in(item[order], doc_off)
    assert own.dtype == torch.float32 and torch.equal(own, m.user_factors)
    # new documents: unknown ids (even ids, 10^6) are dropped, an empty one and one of unknown ids only get zeros
    docs = [[5, 7, 7, 4, 10 ** 6, 9], [], [4, 6], [int(x) for x in items[:30]], [int(items[3])] * 5]
    flat = np.concatenate([np.asarray(d, np.int64) for d in docs])
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    got = m.fold_in(flat, off).cpu().numpy()
    want, d_pos, i_pos = iref.fold_in(Y, items, flat, off, iref.SMALL["alpha"], iref.SMALL["reg"], False, geometry()[0],
                                      segment())
    G64 = iref.gram64(Y)
    assert not got[1].any() and not got[2].any()
    assert sorted(set(d_pos.tolist())) == [0, 3, 4]
    # against fp64 per document, within the float32 restatement's own error
    known = np.isin(flat, items)
    u2, i2, w2 = iref.sum_events(np.repeat(np.arange(len(docs)), np.diff(off))[known], np.searchsorted(items, flat[known]),
                                 None, iref.SMALL["alpha"])
    assert np.array_equal(u2, d_pos) and np.array_equal(i2, i_pos)
    for d in (0, 3, 4):
        x64 = iref.solve_row64(Y, i2[u2 == d], w2[u2 == d], G64, iref.SMALL["reg"], False)
        err_kernel, err_f32 = rel_err(got[d], x64), rel_err(want[d], x64)
        print("fold-in document %d: kernel %.3e float32 restatement %.3e" % (d, err_kernel, err_f32))
        assert err_kernel <= 4 * err_f32 + 8 * ULP32
    # strengths: every id at strength 2 is every id listed twice, bit for bit
    doubled = np.concatenate([np.asarray(d + d, np.int64) for d in docs])
    assert torch.equal(m.fold_in(flat, off, strengths=np.full(len(flat), 2.0)), m.fold_in(doubled, 2 * off))
    with pytest.raises(ValueError, match="strength"):
        m.fold_in(flat, off, strengths=np.zeros(len(flat)))
    with pytest.raises(ValueError, match="doc_offsets"):
        m.fold_in(flat, off[:-1])
    # recommend_documents: fold_in, then recommend's path -- the full-sort oracle on the folded factors
    X = m.fold_in(flat, off).cpu().numpy()
    seen = {d: set(int(x) for x in docs[d]) for d in range(len(docs))}
    k = m.items.numel() - 40
    for exclude in (True, False):
        ids, sc, ln = m.recommend_documents(flat, off, k=k, exclude_seen=exclude, slack=40)       # k' = ni
        w_ids, w_sc, w_ln = iref.recommend(X, Y, range(len(docs)), items, seen, np.arange(len(docs)), k, exclude)
        assert np.array_equal(ln.cpu().numpy(), w_ln) and np.array_equal(ids.cpu().numpy(), w_ids)
        assert np.array_equal(sc.cpu().numpy().view(np.uint32), w_sc.view(np.uint32))
    # the pipeline: split_holdout -> recommend_documents -> ranking_metrics, the split's tensors as they are
    rng = np.random.default_rng(11)
    lens = rng.integers(3, 20, 25)
    ids_all = rng.choice(items, lens.sum()).astype(np.int32)
    offs_all = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    context, c_off, truth, t_off, kept = evaluate.split_holdout(torch.from_numpy(ids_all).to(dev),
                                                                torch.from_numpy(offs_all).to(dev), context=5, min_length=10)
    rec_ids, rec_scores, rec_lengths = m.recommend_documents(context, c_off, k=20)
    assert rec_ids.shape == (kept.numel(), 20) and bool((rec_lengths == 20).all())
    metrics = evaluate.ranking_metrics(rec_ids, rec_lengths, truth, t_off, ks=(1, 10, 20))
    mean = metrics.mean()
    assert mean["n_valid"] == kept.numel() and 0.0 <= float(mean["recall"][-1]) <= 1.0

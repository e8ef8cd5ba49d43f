"""GPU: Bayesian Personalised Ranking (esr_bpr.hip, factorization.BPR) against tests/_bpr_ref.py -- the sampler bit for
bit, the forward / backward and the whole step under the rule of that module (kernel error against fp64 <= 4 e32 + 2^-22),
and the model's refusals, recommendations and learning on the planted corpus."""
import numpy as np
import pytest

import _bpr_ref as bref
from conftest import rel_err

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (1, 2, 63, 64, 65, 1000)


def _dev_csr(csr, dev):
    import torch
    return tuple(torch.from_numpy(a).to(dev) for a in csr)


@pytest.fixture(scope="module")
def boundary_csr():
    """one CSR with a row of every length around the binary search's boundaries, ni = 1001"""
    return bref.random_csr(np.random.default_rng(11), 9, 1001, ROW_LENGTHS), 9, 1001


def _sample(dev, csr, nu, ni, seed, step0, K, B):
    from esrecsys_amd import ops
    return tuple(t.cpu().numpy() for t in ops.bpr_sample(*_dev_csr(csr, dev), nu, ni, seed, step0, K, B))


def _same_draw(got, want, what):
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, "u i j valid dropped".split()[n])


# ---- the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_sampler_equals_the_restatement(dev, boundary_csr, B, K):
    csr, nu, ni = boundary_csr
    seed = (0xC0FFEE << 32) | 99                                              # above 2^32: both key words
    got = _sample(dev, csr, nu, ni, seed, 17, K, B)
    _same_draw(got, bref.sample_ref(*csr, nu, ni, seed, 17, K, B), (B, K))
    assert np.array_equal(got[4], (got[3] == 0).sum(1))


def test_sampler_edge_sizes(dev):
    rng = np.random.default_rng(12)
    cases = [(bref.csr_of({0: [0], 1: []}, 2), 2, 1, 3, 0, 2, 65),            # ni = 1: always dropped
             (bref.csr_of({0: [0], 1: [1], 2: [0, 1]}, 3), 3, 2, 3, 5, 2, 257),   # ni = 2
             (bref.csr_of({2: [4]}, 3), 3, 9, 4, 0, 1, 64),                   # nnz = 1
             (bref.random_csr(rng, 9, 1001, ROW_LENGTHS), 9, 1001, 7, 2 ** 32 - 2, 1, 257),     # the last steps of 2^32
             (bref.random_csr(rng, 40, 12, (0, 1, 11, 12)), 40, 12, 2 ** 64 - 1, 2 ** 32 - 1, 3, 300)]   # the step wraps
    for csr, nu, ni, seed, step0, K, B in cases:
        got = _sample(dev, csr, nu, ni, seed, step0, K, B)
        _same_draw(got, bref.sample_ref(*csr, nu, ni, seed, step0, K, B), (nu, ni, seed, step0))
        assert np.array_equal(got[4], (got[3] == 0).sum(1))
    assert list(_sample(dev, *cases[0])[4]) == [65, 65]


def test_sampler_rows_and_prefixes_do_not_depend_on_the_launch(dev, boundary_csr):
    csr, nu, ni = boundary_csr
    three = _sample(dev, csr, nu, ni, 5, 2 ** 32 - 2, 3, 257)
    for k in range(3):
        one = _sample(dev, csr, nu, ni, 5, (2 ** 32 - 2 + k) % 2 ** 32, 1, 257)
        assert all(np.array_equal(a[k], b[0]) for a, b in zip(three, one)), k
    longer = _sample(dev, csr, nu, ni, 5, 2 ** 32 - 2, 3, 300)
    assert all(np.array_equal(a, b[:, :257]) for a, b in zip(three[:4], longer[:4]))
    assert not np.array_equal(three[2][0], three[2][1])


# ---- forward / backward ----------------------------------------------------------------------------------------------------
def _tables(rng, nu, ni, D):
    """rows of size D^(-1/4) per element: d = x . (yi - yj) is of order 1"""
    s = D ** -0.25
    return (rng.standard_normal((nu, D)) * s).astype(np.float32), (rng.standard_normal((ni, D)) * s).astype(np.float32)


def _run(dev, U, Y, u, i, j, valid, reg, **kw):
    import torch
    from esrecsys_amd import ops
    t = lambda a, dt=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)   # noqa: E731
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.bpr_fwd_bwd(t(U), t(Y), t(u, np.int32), t(i, np.int32), t(j, np.int32), t(valid, np.int32), reg,
                          failed=failed, **kw)
    return tuple(None if o is None else o.cpu().numpy() for o in out) + (int(failed.item()),)


def _check_rule(got, U, Y, u, i, j, valid, reg, what):
    r64 = dict(zip(("loss_t", "d", "grads"), bref.fwd_bwd_ref(U, Y, u, i, j, valid, reg, np.float64)))
    r32 = dict(zip(("loss_t", "d", "grads"), bref.fwd_bwd_ref(U, Y, u, i, j, valid, reg, np.float32)))
    bound, e32 = bref.bounds(r32, r64, ("loss_t", "d", "grads"))
    for k, g in zip(("loss_t", "d", "grads"), got):
        assert np.isfinite(g).all(), (what, k)
        err = rel_err(g, r64[k])
        print("bpr_fwd_bwd %s %s: error %.3g  e32 %.3g  bound %.3g" % (what, k, err, e32[k], bound[k]))
        assert err <= bound[k], (what, k, err, e32[k], bound[k])


@pytest.mark.parametrize("B", [1, 3, 64, 257])
@pytest.mark.parametrize("D", [4, 8, 32, 64, 100, 128])
def test_fwd_bwd_against_fp64(dev, D, B):
    rng = np.random.default_rng([D, B])
    nu, ni = 37, 53
    U, Y = _tables(rng, nu, ni, D)
    for _ in range(50):
        u, i, j = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
        # input condition of the tiny batches: the errors are measured against max |d| of the batch, so a batch of one or
        # three triples takes the first draw whose fp64 |d| are all at least 1 (no cancelled dot product as the yardstick)
        if B > 3 or np.abs(bref.fwd_bwd_ref(U, Y, u, i, j, None, 0.0, np.float64)[1]).min() >= 1.0:
            break
    else:
        raise AssertionError("no draw keeps the input condition")
    if B >= 64:
        j[5:9] = i[5:9]                                                       # i == j
    valid = np.ones(B, np.int32)
    if B >= 3:
        valid[1] = 0
    for reg in (0.0, 0.01):
        loss_t, d, grads, word = _run(dev, U, Y, u, i, j, valid, reg, want_diff=True)
        assert word == 0 and grads.shape == (3 * B, D)
        _check_rule((loss_t, d, grads), U, Y, u, i, j, valid, reg, "D%d-B%d-reg%g" % (D, B, reg))
        off = valid == 0
        assert not loss_t[off].any() and not d[off].any() and not grads[np.tile(off, 3)].any()      # exact zeros
        # no valid array: every triple counts; the valid ones keep their bits
        all_l, all_d, all_g, _ = _run(dev, U, Y, u, i, j, None, reg, want_diff=True)
        keep = ~off
        assert np.array_equal(all_l[keep], loss_t[keep]) and np.array_equal(all_g[np.tile(keep, 3)], grads[np.tile(keep, 3)])
        assert all_l.all() and np.array_equal(all_d[keep], d[keep])


@pytest.mark.parametrize("D", [8, 100])
def test_fwd_bwd_one_user_and_equal_items(dev, D):
    rng = np.random.default_rng(D)
    U, Y = _tables(rng, 5, 40, D)
    B = 130
    u, i = np.full(B, 3), rng.integers(0, 40, B)
    j = np.where(np.arange(B) % 2 == 0, i, rng.integers(0, 40, B))           # every other triple has i == j
    for reg in (0.0, 0.01):
        loss_t, d, grads, word = _run(dev, U, Y, u, i, j, None, reg, want_diff=True)
        assert word == 0
        _check_rule((loss_t, d, grads), U, Y, u, i, j, None, reg, "one-user-D%d-reg%g" % (D, reg))
        same = i == j
        assert not d[same].any() and np.max(np.abs(loss_t[same].astype(np.float64) - np.log(2.0))) <= 2.0 ** -22
        # i == j: the user row's gradient is the regulariser alone, and the item row's two halves sum to it
        assert np.array_equal(grads[:B][same], np.float32(reg) * U[3][None, :].repeat(same.sum(), 0))
        both = grads[B:2 * B][same].astype(np.float64) + grads[2 * B:][same]
        assert np.max(np.abs(both - 2 * np.float32(reg).astype(np.float64) * Y[i[same]])) <= 2.0 ** -22


def test_fwd_bwd_large_score_differences_stay_finite(dev):
    D, B = 32, 121
    rng = np.random.default_rng(60)
    w = rng.standard_normal(D)
    w /= np.linalg.norm(w)
    want = np.linspace(-60.0, 60.0, B)                                        # d = a_t * 7.75 with |a| up to 7.75
    U = (want[:, None] / 7.75 * w[None, :]).astype(np.float32)
    Y = np.concatenate([(7.75 * w)[None, :], np.zeros((1, D))]).astype(np.float32)
    u, i, j = np.arange(B), np.zeros(B, np.int64), np.ones(B, np.int64)
    for reg in (0.0, 0.01):
        loss_t, d, grads, word = _run(dev, U, Y, u, i, j, None, reg, want_diff=True)
        assert word == 0 and abs(d[0] + 60) < 1e-3 and abs(d[-1] - 60) < 1e-3
        assert (loss_t >= 0).all() and loss_t[0] > 59.9 and 0 < loss_t[-1] < 1e-25
        _check_rule((loss_t, d, grads), U, Y, u, i, j, None, reg, "d60-reg%g" % reg)
        if reg == 0.0:
            # g = |g_j| / |x| per triple, against sigmoid(-d) of the kernel's own d in fp64: expf and the division err by
            # a few ulp, g * x rounds once per element -- 16 ulp = 2^-20 relative holds all of it, down to g = e^-60
            keep = np.abs(want) > 1
            g = (np.linalg.norm(grads[2 * B:][keep].astype(np.float64), axis=1)
                 / np.linalg.norm(U[keep].astype(np.float64), axis=1))
            g64 = bref.sigmoid_neg(d[keep].astype(np.float64))
            assert np.max(np.abs(g - g64) / g64) <= 2.0 ** -20


def test_fwd_bwd_forward_only_and_split_batches_keep_their_bits(dev):
    rng = np.random.default_rng(8)
    D, B = 64, 257
    U, Y = _tables(rng, 30, 30, D)
    u, i, j = rng.integers(0, 30, B), rng.integers(0, 30, B), rng.integers(0, 30, B)
    valid = (rng.random(B) < 0.9).astype(np.int32)
    loss_t, d, grads, _ = _run(dev, U, Y, u, i, j, valid, 0.01, want_diff=True)
    f_loss, f_d, f_g, _ = _run(dev, U, Y, u, i, j, valid, 0.01, want_grads=False, want_diff=True)
    assert f_g is None and np.array_equal(f_loss, loss_t) and np.array_equal(f_d, d)
    n_loss, n_d, _, _ = _run(dev, U, Y, u, i, j, valid, 0.01)
    assert n_d is None and np.array_equal(n_loss, loss_t)
    h = 100                                                                   # two halves of other sizes, other lanes
    a = _run(dev, U, Y, u[:h], i[:h], j[:h], valid[:h], 0.01, want_diff=True)
    b = _run(dev, U, Y, u[h:], i[h:], j[h:], valid[h:], 0.01, want_diff=True)
    assert np.array_equal(np.concatenate([a[0], b[0]]), loss_t) and np.array_equal(np.concatenate([a[1], b[1]]), d)
    for part in range(3):
        whole = grads[part * B:(part + 1) * B]
        assert np.array_equal(np.concatenate([a[2][part * h:(part + 1) * h], b[2][part * (B - h):(part + 1) * (B - h)]]), whole)


@pytest.mark.parametrize("D", [4, 100, 128])
def test_fwd_bwd_ids_outside_the_tables(dev, D):
    """the tables sit inside a larger allocation filled with NaN: a read outside them would show"""
    import torch
    from esrecsys_amd import ops
    from esrecsys_amd.factorization import FAIL_BAD_POSITION
    rng = np.random.default_rng(D)
    nu, ni, B, pad = 6, 7, 70, 4 * 1024
    Uh, Yh = _tables(rng, nu, ni, D)
    big = torch.full((2 * pad + (nu + ni) * D + pad,), float("nan"), dtype=torch.float32, device=dev)
    U = big[pad:pad + nu * D].view(nu, D)
    Y = big[2 * pad + nu * D:2 * pad + (nu + ni) * D].view(ni, D)
    U.copy_(torch.from_numpy(Uh))
    Y.copy_(torch.from_numpy(Yh))
    u, i, j = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    u[3], i[10], j[20], u[30], i[40], j[50], u[60] = nu, ni, ni, -1, -1, -1, 2 ** 31 - 1
    bad = np.zeros(B, bool)
    bad[[3, 10, 20, 30, 40, 50, 60]] = True
    t = lambda a: torch.from_numpy(a.astype(np.int32)).to(dev)              # noqa: E731
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    loss_t, d, grads = ops.bpr_fwd_bwd(U, Y, t(u), t(i), t(j), None, 0.01, want_diff=True, failed=failed)
    assert int(failed.item()) == FAIL_BAD_POSITION == 1 << 30
    loss_t, d, grads = loss_t.cpu().numpy(), d.cpu().numpy(), grads.cpu().numpy()
    assert not np.isnan(loss_t).any() and not np.isnan(d).any() and not np.isnan(grads).any()
    assert not loss_t[bad].any() and not d[bad].any() and not grads[np.tile(bad, 3)].any()
    _check_rule((loss_t, d, grads), Uh, Yh, u, i, j, None, 0.01, "bad-ids-D%d" % D)
    # a clean call leaves the word alone
    failed.zero_()
    ops.bpr_fwd_bwd(U, Y, t(u[~bad]), t(i[~bad]), t(j[~bad]), None, 0.01, failed=failed)
    assert int(failed.item()) == 0
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[-pad:]).all())


# ---- the step ----------------------------------------------------------------------------------------------------------------
def _zipf_pairs(rng, nu, ni, per_user):
    p = 1.0 / np.arange(1, ni + 1) ** 1.1
    p /= p.sum()
    # every other user has one event, the rest 2 per_user - 1: the short rows are often named by no triple of a few steps
    user = np.repeat(np.arange(nu), np.where(np.arange(nu) % 2 == 0, 1, 2 * per_user - 1))
    item = rng.choice(ni, user.size, p=p)                                    # repeated pairs collapse in the model
    every = np.arange(ni)                                                    # and every item is seen by somebody
    return np.concatenate([user, every % nu]), np.concatenate([item, every])


STEP = dict(nu=200, ni=300, rank=32, batch=257)


def _step_model(dev, optimizer, seed=4):
    from esrecsys_amd.factorization import BPR
    user, item = _zipf_pairs(np.random.default_rng(21), STEP["nu"], STEP["ni"], 12)
    return BPR(user, item, rank=STEP["rank"], batch=STEP["batch"], optimizer=optimizer, seed=seed, device=dev)


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_train_steps_equal_the_ops_composed_by_hand(dev, optimizer):
    import torch
    from esrecsys_amd import ops
    a, b = _step_model(dev, optimizer), _step_model(dev, optimizer)
    nu, ni, B = STEP["nu"], STEP["ni"], STEP["batch"]
    assert torch.equal(a.user_factors, b.user_factors) and a.nnz == b.nnz < nu * 12 + ni
    assert (a.users.numel(), a.items.numel()) == (nu, ni)
    losses = a.train_steps(5)
    u, i, j, valid, dropped = ops.bpr_sample(b._offsets_dev, b._row_upos, b._row_ipos, nu, ni, b.seed, 0, 5, B)
    by_hand = []
    for k in range(5):
        loss_t, _, grads = ops.bpr_fwd_bwd(b.user_factors, b.item_factors, u[k], i[k], j[k], valid[k], b.reg)
        if optimizer == "adagrad":
            s, p = ops.segment_sort_multi([u[k], i[k], j[k]], [0, nu, nu], nu + ni)
            ops.sparse_adagrad_multi([b.user_factors, b.item_factors], [b.user_accum, b.item_accum], [0, nu, nu + ni], s, p,
                                     grads, b.lr)
        else:
            s, p = ops.segment_sort(u[k], nu)
            ops.sparse_sgd(b.user_factors, s, p, grads[:B], b.lr)
            s, p = ops.segment_sort(torch.cat([i[k], j[k]]), ni)
            ops.sparse_sgd(b.item_factors, s, p, grads[B:], b.lr)
        by_hand.append(float(loss_t.to(torch.float64).sum()) / (B - int(dropped[k])))
    assert losses == by_hand and a.step == 5 and b.step == 0
    for x, y in ((a.user_factors, b.user_factors), (a.item_factors, b.item_factors), (a.user_accum, b.user_accum),
                 (a.item_accum, b.item_accum)):
        assert torch.equal(x, y)
    # the next call goes on at step 5
    assert all(torch.equal(x, y) for x, y in zip(a.sample(2), a.sample(2, step0=5)))


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_five_steps_against_fp64(dev, optimizer):
    m = _step_model(dev, optimizer)
    nu, ni, B = STEP["nu"], STEP["ni"], STEP["batch"]
    assert (m.users.numel(), m.items.numel()) == (nu, ni)
    start = {k: getattr(m, a).cpu().numpy() for k, a in (("user", "user_factors"), ("item", "item_factors"),
                                                         ("user_acc", "user_accum"), ("item_acc", "item_accum"))}
    u, i, j, valid, _ = (t.cpu().numpy() for t in m.sample(5))
    csr = (m._user_offsets, m._row_upos.cpu().numpy(), m._row_ipos.cpu().numpy())
    _same_draw((u, i, j, valid), bref.sample_ref(*csr, nu, ni, m.seed, 0, 5, B)[:4], "step")
    assert len(np.unique(i)) < i.size // 4                                   # Zipf items: ids repeat
    losses = m.train_steps(5)
    state = {np.float64: dict(start), np.float32: dict(start)}
    ref_losses = {np.float64: [], np.float32: []}
    for dtype, s in state.items():
        for k in range(5):
            r = bref.step_ref(s["user"], s["item"], s["user_acc"], s["item_acc"], u[k], i[k], j[k], valid[k], m.reg, m.lr,
                              optimizer, dtype)
            s.update({key: r[key] for key in ("user", "item", "user_acc", "item_acc")})
            ref_losses[dtype].append(r["loss"])
    keys = ("user", "item") + (("user_acc", "item_acc") if optimizer == "adagrad" else ())
    bound, e32 = bref.bounds(state[np.float32], state[np.float64], keys)
    got = {"user": m.user_factors, "item": m.item_factors, "user_acc": m.user_accum, "item_acc": m.item_accum}
    for key in keys:
        err = rel_err(got[key].cpu().numpy(), state[np.float64][key])
        print("bpr step %s %s: error %.3g  e32 %.3g  bound %.3g" % (optimizer, key, err, e32[key], bound[key]))
        assert err <= bound[key], (key, err, e32[key], bound[key])
    for k in range(5):
        e = abs(ref_losses[np.float32][k] - ref_losses[np.float64][k]) / ref_losses[np.float64][k]
        err = abs(losses[k] - ref_losses[np.float64][k]) / ref_losses[np.float64][k]
        print("bpr step %s loss %d: error %.3g  e32 %.3g" % (optimizer, k, err, e))
        assert err <= bref.FACTOR * e + bref.FLOOR, (k, err, e)
    if optimizer == "sgd":
        assert np.array_equal(m.user_accum.cpu().numpy(), start["user_acc"])
    # rows that no triple names keep their bits: after the five steps (users with one pair are often not drawn; the
    # negatives of 1285 triples cover all the items), and after one step of a fresh model, where items are left out too
    one = _step_model(dev, optimizer)
    u1, i1, j1, _, _ = (t.cpu().numpy() for t in one.sample(1))
    one.train_steps(1)
    for model, uu, ij, need_items in ((m, u, np.concatenate([i, j]), False), (one, u1, np.concatenate([i1, j1]), True)):
        for key, ids, n, need in (("user", uu, nu, True), ("item", ij, ni, need_items)):
            quiet = np.setdiff1d(np.arange(n), ids)
            assert quiet.size or not need, key
            now = {"user": model.user_factors, "item": model.item_factors, "user_acc": model.user_accum,
                   "item_acc": model.item_accum}
            assert np.array_equal(now[key].cpu().numpy()[quiet], start[key][quiet])
            assert np.array_equal(now[key + "_acc"].cpu().numpy()[quiet], start[key + "_acc"][quiet])
            named = np.unique(ids)
            assert not np.array_equal(now[key].cpu().numpy()[named], start[key][named])


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_constructor_on_the_device(dev):
    import torch
    from esrecsys_amd.factorization import BPR
    for bad in ([-1, 2], [2 ** 31 - 1, 2]):
        with pytest.raises(ValueError, match="2\\^31 - 1"):
            BPR(bad, [0, 1], rank=4, device=dev)
        with pytest.raises(ValueError, match="2\\^31 - 1"):
            BPR([0, 1], bad, rank=4, device=dev)
    m = BPR([7, 7, 7, 3, 7], [5, 9, 5, 5, 5], rank=4, batch=8, seed=2, device=dev)          # repeated events collapse
    assert m.nnz == 3 and m.users.tolist() == [3, 7] and m.items.tolist() == [5, 9] and m.step == 0
    assert m._user_offsets.tolist() == [0, 1, 3] and m._row_upos.tolist() == [0, 1, 1] and m._row_ipos.tolist() == [0, 0, 1]
    assert m._key.tolist() == [0, (1 << 32), (1 << 32) | 1]
    gen = torch.Generator(device="cpu").manual_seed(2)
    assert torch.equal(m.user_factors.cpu(), torch.randn(2, 4, generator=gen) * 0.5)
    assert torch.equal(m.item_factors.cpu(), torch.randn(2, 4, generator=gen) * 0.5)
    d = BPR.from_documents([7, 2, 7, 7, 5], [0, 3, 3, 5], rank=4, batch=8, init_scale=0.25, device=dev)
    assert d.users.tolist() == [0, 2] and d.items.tolist() == [2, 5, 7] and d.nnz == 4 and d.init_scale == 0.25
    u, i, j, valid, dropped = d.sample(3)
    assert tuple(u.shape) == (3, 8) and tuple(dropped.shape) == (3,)
    # a user who has seen both items: every triple is dropped, and a step of nothing but dropped triples has no loss
    one = BPR([1, 1], [0, 1], rank=4, batch=16, device=dev)
    before = one.user_factors.clone()
    assert np.isnan(one.train_steps(2)).all() and torch.equal(one.user_factors, before) and np.isnan(one.auc())


def test_recommend_equals_a_full_sort_of_the_scores(dev):
    import torch
    from esrecsys_amd.factorization import BPR
    rng = np.random.default_rng(31)
    user, item = _zipf_pairs(rng, 30, 45, 6)
    m = BPR(user * 3 + 1, item * 2, rank=8, batch=128, device=dev)          # ids are not positions
    m.train_steps(3)
    # equal rows: equal scores, ordered by item id
    m.item_factors[7] = m.item_factors[3]
    m.item_factors[20] = m.item_factors[3]
    queries = np.array([1, 4, 2, 88, 1000, 4], np.int64)                      # 2 and 1000 are unknown
    items = m.items.cpu().numpy().astype(np.int64)
    table = m.score(np.repeat(queries, items.size), np.tile(items, queries.size)).cpu().numpy().reshape(queries.size, -1)
    seen = set(zip((user * 3 + 1).tolist(), (item * 2).tolist()))
    k = 10
    for exclude in (True, False):
        ids, scores, lengths = (t.cpu().numpy() for t in m.recommend(queries, k=k, exclude_seen=exclude))
        for q, uid in enumerate(queries):
            if uid not in m.users.tolist():
                assert lengths[q] == 0 and (ids[q] == -1).all() and not scores[q].any() and np.isnan(table[q]).all()
                continue
            cand = [(-table[q, c], int(items[c])) for c in range(items.size) if not (exclude and (uid, int(items[c])) in seen)]
            order = sorted(cand)[:k]
            assert lengths[q] == len(order) == k
            assert ids[q].tolist() == [c[1] for c in order], (q, exclude)
            assert scores[q].view(np.int32).tolist() == np.array([-c[0] for c in order], np.float32).view(np.int32).tolist()
    assert torch.equal(m.score([1, 1], [0, 1]).isnan().cpu(), torch.tensor([False, True]))


def test_planted_corpus_learning_auc_and_metrics(dev):
    from esrecsys_amd import evaluate
    from esrecsys_amd.factorization import BPR
    P = bref.PLANTED
    user, item = bref.planted_pairs()
    m = BPR(user, item, rank=P["rank"], batch=P["batch"], reg=bref.REG, lr=bref.LR, seed=P["seed"], device=dev)
    before = m.auc(K=4)
    assert 0.0 <= before <= 1.0 and m.auc(K=4) == before and m.step == 0
    losses = m.fit(P["steps"])
    assert len(losses) == P["steps"] == m.step and np.isfinite(losses).all()
    assert np.mean(losses[-10:]) < np.mean(losses[:10]), (losses[:10], losses[-10:])
    after = m.auc(K=4)
    print("bpr planted corpus: loss %.4f -> %.4f, auc %.4f -> %.4f" % (np.mean(losses[:10]), np.mean(losses[-10:]), before,
                                                                      after))
    assert after > before
    # the lists go into ranking_metrics as they are; the truth: the unseen items of the user's own half
    import torch
    users = np.arange(P["nu"])
    ids, scores, lengths = m.recommend(users, k=10)
    truth, offsets = [], [0]
    for u in users:
        own = set(range(32 * (u >= 32), 32 * (u >= 32) + 32)) - set(item[user == u].tolist())
        truth += sorted(own)
        offsets.append(len(truth))
    metrics = evaluate.ranking_metrics(ids, lengths, torch.tensor(truth, dtype=torch.int32, device=dev),
                                       torch.tensor(offsets, dtype=torch.int64, device=dev), ks=(10,)).mean()
    print("bpr planted corpus: precision@10 %.3f (24 of 56 unseen items are the user's half)" % metrics["precision"][0])
    assert metrics["n_valid"] == P["nu"] and 0.0 < metrics["precision"][0] <= 1.0
    assert int(lengths.min()) == 10 and int(ids.min()) >= 0 and ids.dtype == torch.int32

"""GPU: the bag kernels (esr_bag.hip) and factorization.HybridBPR against tests/_hybrid_ref.py -- both kernels bit for bit on
exact tables over the grid of widths, row counts and bag lengths, independent of the launch, within the rule of that module
(kernel error against fp64 <= 4 e32 + 2^-22) on random tables and over whole steps, the refusals, train_steps against the
calls composed by hand, the identity-only model against BPR, and cold-start learning on the planted corpus.

Measured on an MI355X (profiles/hybrid/parity_errors.json): see DESIGN.md section 4l."""
import json
import os

import numpy as np
import pytest

import _bpr_ref as bref
import _hybrid_ref as href
from conftest import rel_err

pytestmark = pytest.mark.gpu

DS = (4, 8, 32, 64, 100, 128)
NS = (1, 63, 64, 65, 257)
N_BAGS, NF = 257, 50
MEASURED = {}


def _t(a, dev, dt=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def grid():
    """per D: the exact table, the 257 bags (every length of href.LENGTHS, witnesses placed across any unroll) and the
    float32-chain restatement of every bag with and without weights -- computed once, shared and left unchanged"""
    out = {}
    for D in DS:
        rng = np.random.default_rng(D)
        table = href.exact_table(rng, NF, D)
        off, feat, w = href.grid_bags(rng, N_BAGS, NF)
        want = {flag: href.bag_sum_ref(table, off, feat, w if flag else None, None, np.float32)[0] for flag in (False, True)}
        out[D] = (table, off, feat, w, want)
    lens = np.diff(out[4][1])
    assert lens.min() == 0 and lens.max() > 1024 and set(lens.tolist()) == set(href.LENGTHS)
    # the witness triples start at every residue mod 8 among the bags longer than 64
    starts = [int(np.flatnonzero(out[4][2][out[4][1][b]:out[4][1][b + 1]] == NF)[0]) for b in np.flatnonzero(lens > 64)]
    assert {s % 8 for s in starts} == set(range(8))
    return out


def _rows_cases(n, rng):
    """rows = None over the first n bags, a permutation of n distinct bags, n draws with repeats"""
    perm = rng.permutation(N_BAGS)[:n].astype(np.int32)
    rep = rng.integers(0, min(N_BAGS, 24), n).astype(np.int32)
    if n > 1:
        rep[-1] = rep[0]
    return {"null": None, "permutation": perm, "repeats": rep}


def _sum(dev, table, off, feat, w, rows, n_bags=None):
    import torch
    from esrecsys_amd import ops
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    o = off if n_bags is None else off[:n_bags + 1]
    out = ops.bag_sum(_t(table, dev), _t(o, dev), _t(feat, dev), _t(w, dev), rows=_t(rows, dev, np.int32), failed=failed)
    return out.cpu().numpy(), int(failed.item())


def _expand(dev, table, off, feat, w, rows, g, valid, reg, n_bags=None):
    import torch
    from esrecsys_amd import ops
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    o = off if n_bags is None else off[:n_bags + 1]
    oo = href.out_offsets_ref(o, rows, feat.size)
    f, rows_out = ops.bag_expand(_t(table, dev), _t(o, dev), _t(feat, dev), _t(w, dev), _t(rows, dev, np.int32), _t(g, dev),
                                 _t(valid, dev, np.int32), _t(oo, dev), int(oo[-1]), reg, failed=failed)
    return f.cpu().numpy(), rows_out.cpu().numpy(), int(failed.item())


# ---- the exact grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_exact_grid_bit_for_bit(dev, grid, D, n):
    table, off, feat, w, want = grid[D]
    rng = np.random.default_rng([D, n])
    cases = _rows_cases(n, rng)
    assert n == 1 or len(set(cases["repeats"].tolist())) < n                 # a repeated row
    lens = np.diff(off)
    if n >= 63:
        picked = np.concatenate([cases["permutation"], cases["repeats"]])
        assert lens[picked].max() > 1024 and lens[picked].min() == 0        # a bag longer than 1024 and an empty one
    for name, rows in cases.items():
        sel = np.arange(n) if rows is None else rows
        nb = n if rows is None else None
        for flag in (False, True):
            got, word = _sum(dev, table, off, feat, w if flag else None, rows, nb)
            assert word == 0 and got.shape == (n, D)
            assert np.array_equal(_bits(got), _bits(want[flag][sel])), ("sum", name, flag)
            g = href.exact_table(rng, n, D)[:n]
            mixed = (rng.random(n) < 0.6).astype(np.int32)
            mixed[0] = 0
            for valid in (None, mixed):
                f, rows_out, word = _expand(dev, table, off, feat, w if flag else None, rows, g, valid, 0.25, nb)
                o = off if nb is None else off[:nb + 1]
                wf, wrows, _, wfailed = href.bag_expand_ref(table, o, feat, w if flag else None, rows, g, valid, 0.25, np.float32)
                assert word == 0 and not wfailed and f.dtype == np.int32 and np.array_equal(f, wf), ("expand", name, flag)
                assert np.array_equal(_bits(rows_out), _bits(wrows)), ("expand", name, flag, valid is None)
                if valid is not None:
                    dead = np.repeat(mixed == 0, lens[sel])
                    assert dead.any() or lens[sel[mixed == 0]].sum() == 0
                    assert not rows_out[dead].any()


def test_hand_worked_bags_on_the_device(dev):
    big = 2.0 ** 25
    table = np.repeat(np.array([big, 1.0, -big, 3.5], np.float32)[:, None], 8, 1)
    off = np.array([0, 3, 3, 4, 7, 10], np.int64)
    feat = np.array([0, 1, 2, 3, 0, 2, 1, 1, 0, 2], np.int32)
    got, word = _sum(dev, table, off, feat, None, None)
    assert word == 0
    assert not got[0].any() and not got[1].any() and not np.signbit(got[1]).any()       # the stated order; the empty bag
    assert np.array_equal(got[2], table[3])                                              # identity-only: the row itself
    assert (got[3] == 1.0).all() and not got[4].any()                                    # (2^25, -2^25, 1) and (1, 2^25, -2^25)


# ---- launch independence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 100])
def test_subsets_prefixes_and_split_calls_keep_their_bits(dev, grid, D):
    table, off, feat, w, want = grid[D]
    rng = np.random.default_rng(D + 1)
    rows = rng.integers(0, N_BAGS, 300).astype(np.int32)
    g = href.exact_table(rng, 300, D)[:300]
    valid = (rng.random(300) < 0.7).astype(np.int32)
    whole, _ = _sum(dev, table, off, feat, w, rows)
    ef, er, _ = _expand(dev, table, off, feat, w, rows, g, valid, 0.25)
    oo = href.out_offsets_ref(off, rows)
    assert np.array_equal(_bits(whole), _bits(want[True][rows]))
    for part in (slice(0, 77), slice(77, 300), np.arange(0, 300, 3)):
        got, _ = _sum(dev, table, off, feat, w, rows[part])
        assert np.array_equal(_bits(got), _bits(whole[part]))
    a = _expand(dev, table, off, feat, w, rows[:77], g[:77], valid[:77], 0.25)
    b = _expand(dev, table, off, feat, w, rows[77:], g[77:], valid[77:], 0.25)
    assert np.array_equal(np.concatenate([a[0], b[0]]), ef) and np.array_equal(_bits(np.concatenate([a[1], b[1]])), _bits(er))
    assert a[0].size == oo[77]


@pytest.mark.parametrize("D", [4, 128])
def test_past_the_launch_grid(dev, D):
    """the grid is capped at 2048 workgroups of 256 / G groups: bags of one and two occurrences go past it, bit for bit"""
    G = 1
    while G < D // 4:
        G *= 2
    n = 2048 * (256 // G) + 2 * (256 // G) + 3
    rng = np.random.default_rng(D)
    nf = 64
    table = href.exact_table(rng, nf, D)
    lens = rng.integers(1, 3, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feat = rng.integers(0, nf, int(off[-1])).astype(np.int32)
    w = href.exact_weights(rng, feat.size)
    want, _ = href.bag_sum_ref(table, off, feat, w, None, np.float32)
    got, word = _sum(dev, table, off, feat, w, None)
    assert word == 0 and np.array_equal(_bits(got), _bits(want))
    rows = rng.permutation(n).astype(np.int32)
    got, word = _sum(dev, table, off, feat, w, rows)
    assert word == 0 and np.array_equal(_bits(got), _bits(want[rows]))
    g = table[rng.integers(0, nf, n)]
    valid = (rng.random(n) < 0.8).astype(np.int32)
    f, rows_out, word = _expand(dev, table, off, feat, w, rows, g, valid, 0.25)
    wf, wrows, _, _ = href.bag_expand_ref(table, off, feat, w, rows, g, valid, 0.25, np.float32)
    assert word == 0 and np.array_equal(f, wf) and np.array_equal(_bits(rows_out), _bits(wrows))


# ---- random tables: the rule ---------------------------------------------------------------------------------------------------
def _note(key, err, e32=None):
    """keep a measured error (with its multiple of e32 and its share of the bound) or, without e32, a plain figure"""
    MEASURED[key] = err if e32 is None else {"error": err, "e32": e32, "multiple_of_e32": err / e32 if e32 else 0.0,
                                             "share_of_bound": err / (href.FACTOR * e32 + href.FLOOR)}
    path = os.environ.get("ESR_HYBRID_PARITY_JSON")     # (profiles/hybrid/parity_errors.json is one run written this way)
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


def _within(key, got, r32, r64):
    e32 = bref.arr_err(r32, r64)
    err = rel_err(got, r64)
    print("hybrid %s: error %.3g  e32 %.3g  bound %.3g" % (key, err, e32, href.FACTOR * e32 + href.FLOOR))
    _note(key, err, e32)
    assert np.isfinite(got).all() and err <= href.FACTOR * e32 + href.FLOOR, (key, err, e32)


@pytest.mark.parametrize("D", [8, 64, 100])
def test_random_tables_against_fp64(dev, D):
    rng = np.random.default_rng(D)
    nf, n_bags, n = 300, 64, 257
    table = (rng.standard_normal((nf, D)) * D ** -0.25).astype(np.float32)
    off, feat, _ = href.grid_bags(rng, n_bags, nf - 3)
    w = rng.standard_normal(feat.size).astype(np.float32)
    rows = rng.integers(0, n_bags, n).astype(np.int32)
    got, word = _sum(dev, table, off, feat, w, rows)
    assert word == 0
    _within("bag_sum-D%d" % D, got, href.bag_sum_ref(table, off, feat, w, rows, np.float32)[0],
            href.bag_sum_ref(table, off, feat, w, rows, np.float64)[0])
    g = rng.standard_normal((n, D)).astype(np.float32)
    valid = (rng.random(n) < 0.8).astype(np.int32)
    f, rows_out, word = _expand(dev, table, off, feat, w, rows, g, valid, 0.01)
    r32 = href.bag_expand_ref(table, off, feat, w, rows, g, valid, 0.01, np.float32)
    r64 = href.bag_expand_ref(table, off, feat, w, rows, g, valid, 0.01, np.float64)
    assert word == 0 and np.array_equal(f, r64[0])
    _within("bag_expand-D%d" % D, rows_out, r32[1], r64[1])


# ---- refusals --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 100])
def test_positions_outside_the_tables(dev, D):
    """the table sits inside a larger allocation filled with NaN: a read outside it would show.  Every index stays inside
    the allocated arrays."""
    import torch
    from esrecsys_amd import ops
    from esrecsys_amd.factorization import FAIL_BAD_POSITION
    rng = np.random.default_rng(D)
    nf, pad = 20, 4 * 1024
    host = href.exact_table(rng, nf - 3, D)
    big = torch.full((2 * pad + nf * D,), float("nan"), dtype=torch.float32, device=dev)
    table = big[pad:pad + nf * D].view(nf, D)
    table.copy_(torch.from_numpy(host))
    off = np.array([0, 3, 5, 5, 9, 12], np.int64)
    feat = np.array([1, 2, 3, nf, 4, 5, -1, 6, 7, 8, 9, 2 ** 31 - 1], np.int32)     # bags 1, 3 and 4 name a bad position
    rows = np.array([0, 1, 2, 5, 3, -1, 4, 0], np.int32)                             # rows 3 and 5 name a bad bag
    bad = np.array([False, True, False, True, True, True, True, False])
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.bag_sum(table, _t(off, dev), _t(feat, dev), None, rows=_t(rows, dev), failed=failed).cpu().numpy()
    assert int(failed.item()) == FAIL_BAD_POSITION == 1 << 30
    want, wfailed = href.bag_sum_ref(host, off, feat, None, rows, np.float32)
    assert wfailed and not np.isnan(out).any() and not out[bad].any() and np.array_equal(_bits(out), _bits(want))
    assert out[0].any() and np.array_equal(out[0], out[7])
    g = href.exact_table(rng, 8, D)[:8]
    oo = href.out_offsets_ref(off, rows)
    failed.zero_()
    f, rows_out = ops.bag_expand(table, _t(off, dev), _t(feat, dev), None, _t(rows, dev), _t(g, dev), None, _t(oo, dev),
                                 int(oo[-1]), 0.25, failed=failed)
    wf, wrows, _, wfailed = href.bag_expand_ref(host, off, feat, None, rows, g, None, 0.25, np.float32)
    assert int(failed.item()) == 1 << 30 and wfailed
    f, rows_out = f.cpu().numpy(), rows_out.cpu().numpy()
    assert np.array_equal(f, wf) and not np.isnan(rows_out).any() and np.array_equal(_bits(rows_out), _bits(wrows))
    refused = np.isin(np.concatenate([feat[off[b]:off[b + 1]] for b in rows if 0 <= b < 5]), [nf, -1, 2 ** 31 - 1])
    assert refused.sum() == 3 and not rows_out[refused].any() and not f[refused].any() and rows_out[~refused].any(1).all()
    # a clean call leaves the word alone
    failed.zero_()
    ops.bag_sum(table, _t(off[:2], dev), _t(feat, dev), None, failed=failed)
    assert int(failed.item()) == 0
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[-pad:]).all())


# ---- the model ---------------------------------------------------------------------------------------------------------------
STEP = dict(nu=120, ni=200, rank=32, batch=257)


def _pairs(rng):
    nu, ni = STEP["nu"], STEP["ni"]
    p = 1.0 / np.arange(1, ni + 1) ** 1.1
    user = np.repeat(np.arange(nu), 9)
    item = rng.choice(ni, user.size, p=p / p.sum())
    every = np.arange(ni)
    return np.concatenate([user, every % nu]), np.concatenate([item, every])


def _features(rng):
    """items: one feature shared by EVERY item (a run of 2 B occurrences for the combiner), a category, some tags with
    weights; users: a group feature for every other user"""
    ni, nu = STEP["ni"], STEP["nu"]
    ent = [np.arange(ni), np.arange(ni)]
    fid = [np.full(ni, 7), 1000 + np.arange(ni) % 9]
    for i in range(0, ni, 3):
        tags = rng.choice(30, rng.integers(1, 5), replace=False)
        ent.append(np.full(tags.size, i))
        fid.append(2000 + tags)
    ent, fid = np.concatenate(ent), np.concatenate(fid)
    weight = (2.0 ** rng.integers(-2, 2, ent.size)).astype(np.float32)
    users = np.arange(0, nu, 2)
    return (ent, fid, weight), (users, 50 + users % 5, None)


def _model(dev, optimizer, identity=(True, True), seed=4):
    from esrecsys_amd.factorization import HybridBPR
    user, item = _pairs(np.random.default_rng(21))
    item_features, user_features = _features(np.random.default_rng(22))
    return HybridBPR(user, item, user_features=user_features, item_features=item_features, identity=identity,
                     rank=STEP["rank"], batch=STEP["batch"], optimizer=optimizer, seed=seed, device=dev)


def test_constructor_on_the_device(dev):
    import torch
    from esrecsys_amd.factorization import BPR, HybridBPR
    m = HybridBPR([7, 7, 3], [5, 9, 5], item_features=([9, 5, 9], [40, 40, 30], [2.0, 0.5, 4.0]), rank=4, batch=8, seed=2,
                  device=dev)
    assert m.users.tolist() == [3, 7] and m.items.tolist() == [5, 9] and m.item_feature_ids.tolist() == [30, 40]
    assert m.user_feature_ids.numel() == 0 and tuple(m.user_embeddings.shape) == (2, 4) and tuple(m.item_embeddings.shape) == (4, 4)
    assert m._item_bags.offsets.tolist() == [0, 2, 5] and m._item_bags.feat.tolist() == [0, 3, 1, 2, 3]
    assert m._item_bags.weight.tolist() == [1.0, 0.5, 1.0, 4.0, 2.0] and m._user_bags.weight is None
    gen = torch.Generator(device="cpu").manual_seed(2)
    assert torch.equal(m.user_embeddings.cpu(), torch.randn(2, 4, generator=gen) * 0.5)
    assert torch.equal(m.item_embeddings.cpu(), torch.randn(4, 4, generator=gen) * 0.5)
    e = m.item_embeddings.cpu().numpy().astype(np.float64)
    want = np.stack([e[0] + 0.5 * e[3], e[1] + 4.0 * e[2] + 2.0 * e[3]])
    assert np.max(np.abs(m.item_rows().cpu().numpy() - want)) <= 1e-6 and torch.equal(m.user_rows(), m.user_embeddings)
    # identity-only: BPR's tables, bit for bit
    a, b = HybridBPR([7, 7, 3], [5, 9, 5], rank=4, batch=8, seed=2, device=dev), BPR([7, 7, 3], [5, 9, 5], rank=4, batch=8,
                                                                                      seed=2, device=dev)
    assert torch.equal(a.user_factors, b.user_factors) and torch.equal(a.item_factors, b.item_factors)
    # no identity on the item side: features only
    c = HybridBPR([7, 7, 3], [5, 9, 5], item_features=([9, 5], [40, 30], None), identity=(True, False), rank=4, batch=8,
                  device=dev)
    assert tuple(c.item_embeddings.shape) == (2, 4) and c._item_bags.feat.tolist() == [0, 1]
    with pytest.raises(ValueError, match="never|not seen"):
        m.compose_items([11], [41])
    with pytest.raises(ValueError, match="was in training"):
        m.compose_items([9], [40])
    ids, rows = m.compose_items([12, 11, 12], [40, 30, 30], [1.0, 2.0, 3.0])
    assert ids.tolist() == [11, 12] and np.max(np.abs(rows.cpu().numpy() - np.stack([2.0 * e[2], 3.0 * e[2] + e[3]]))) <= 1e-6


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_train_steps_equal_the_ops_composed_by_hand(dev, optimizer):
    import torch
    from esrecsys_amd import ops
    a, b = _model(dev, optimizer), _model(dev, optimizer)
    B, K = STEP["batch"], 4
    nfu, nfi = b.user_embeddings.shape[0], b.item_embeddings.shape[0]
    assert nfu == STEP["nu"] + 5 and nfi == STEP["ni"] + 1 + 9 + b.item_feature_ids.numel() - 10
    assert int((b._item_bags.feat == STEP["ni"]).sum()) == STEP["ni"]        # the feature every item shares (id 7 is least)
    losses = a.train_steps(K)
    u, i, j, valid, dropped = b.sample(K)
    ar = torch.arange(2 * B, dtype=torch.int32, device=dev)
    by_hand = []
    for k in range(K):
        ij, v2 = torch.cat([i[k], j[k]]), torch.cat([valid[k], valid[k]])
        P = ops.bag_sum(b.user_embeddings, *b._user_bags.args(), rows=u[k])
        Q = ops.bag_sum(b.item_embeddings, *b._item_bags.args(), rows=ij)
        loss_t, _, grads = ops.bpr_fwd_bwd(P, Q, ar[:B], ar[:B], ar[B:], valid[k], 0.0)
        oo_u = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(b._user_bags.lengths[u[k].long()], 0)])
        oo_i = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(b._item_bags.lengths[ij.long()], 0)])
        fu, gu = ops.bag_expand(b.user_embeddings, *b._user_bags.args(), u[k], grads[:B], valid[k], oo_u, int(oo_u[-1]), b.reg)
        fi, gi = ops.bag_expand(b.item_embeddings, *b._item_bags.args(), ij, grads[B:], v2, oo_i, int(oo_i[-1]), b.reg)
        assert int((fi == STEP["ni"]).sum()) == 2 * B                        # the long run
        if optimizer == "adagrad":
            s, p = ops.segment_sort_multi([fu, fi], [0, nfu], nfu + nfi)
            ops.sparse_adagrad_multi([b.user_embeddings, b.item_embeddings], [b.user_accum, b.item_accum], [0, nfu, nfu + nfi],
                                     s, p, torch.cat([gu, gi]), b.lr)
        else:
            s, p = ops.segment_sort(fu, nfu)
            ops.sparse_sgd(b.user_embeddings, s, p, gu, b.lr)
            s, p = ops.segment_sort(fi, nfi)
            ops.sparse_sgd(b.item_embeddings, s, p, gi, b.lr)
        by_hand.append(float(loss_t.to(torch.float64).sum()) / (B - int(dropped[k])))
    assert losses == by_hand and a.step == K and b.step == 0
    for x, y in ((a.user_embeddings, b.user_embeddings), (a.item_embeddings, b.item_embeddings), (a.user_accum, b.user_accum),
                 (a.item_accum, b.item_accum)):
        assert torch.equal(x, y)
    assert not torch.equal(a.item_embeddings, _model(dev, optimizer).item_embeddings)
    # the composed tables follow the step
    assert torch.equal(a.item_rows(), ops.bag_sum(b.item_embeddings, *b._item_bags.args()))


def _host_state(m):
    return {"user": m.user_embeddings.cpu().numpy(), "item": m.item_embeddings.cpu().numpy(),
            "user_acc": m.user_accum.cpu().numpy(), "item_acc": m.item_accum.cpu().numpy()}


def _host_bags(m):
    return tuple(tuple(None if t is None else t.cpu().numpy() for t in bags.args()) for bags in (m._user_bags, m._item_bags))


def _reference_steps(start, ubag, ibag, u, i, j, valid, reg, lr, optimizer, K):
    state = {np.float64: dict(start), np.float32: dict(start)}
    losses = {np.float64: [], np.float32: []}
    for dtype, s in state.items():
        for k in range(K):
            r = href.step_ref(s["user"], s["item"], s["user_acc"], s["item_acc"], ubag, ibag, u[k], i[k], j[k], valid[k], reg,
                              lr, optimizer, dtype)
            s.update({key: r[key] for key in ("user", "item", "user_acc", "item_acc")})
            losses[dtype].append(r["loss"])
    return state, losses


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_one_whole_step_against_fp64(dev, optimizer):
    m = _model(dev, optimizer)
    start, (ubag, ibag) = _host_state(m), _host_bags(m)
    u, i, j, valid, _ = (t.cpu().numpy() for t in m.sample(1))
    losses = m.train_steps(1)
    state, ref_losses = _reference_steps(start, ubag, ibag, u, i, j, valid, m.reg, m.lr, optimizer, 1)
    got = _host_state(m)
    for key in ("user", "item") + (("user_acc", "item_acc") if optimizer == "adagrad" else ()):
        _within("step-%s-%s" % (optimizer, key), got[key], state[np.float32][key], state[np.float64][key])
    e = abs(ref_losses[np.float32][0] - ref_losses[np.float64][0]) / ref_losses[np.float64][0]
    err = abs(losses[0] - ref_losses[np.float64][0]) / ref_losses[np.float64][0]
    print("hybrid step %s loss: error %.3g  e32 %.3g" % (optimizer, err, e))
    assert err <= href.FACTOR * e + href.FLOOR
    if optimizer == "sgd":
        assert np.array_equal(got["user_acc"], start["user_acc"])
    # features that no bag of the step names keep their bits
    named = np.unique(np.concatenate([ibag[1][ibag[0][b]:ibag[0][b + 1]] for b in np.concatenate([i[0], j[0]])]))
    quiet = np.setdiff1d(np.arange(start["item"].shape[0]), named)
    assert quiet.size and np.array_equal(got["item"][quiet], start["item"][quiet])
    assert not np.array_equal(got["item"][named], start["item"][named])


def test_identity_only_model_against_bpr(dev):
    """same seed, same pairs: five steps of both models stay within the rule of the fp64 restatement, and their auc agree
    to what that bound lets a score difference move"""
    import torch
    from esrecsys_amd.factorization import BPR, HybridBPR
    user, item = _pairs(np.random.default_rng(21))
    kw = dict(rank=STEP["rank"], batch=STEP["batch"], seed=4, device=dev)
    h, b = HybridBPR(user, item, **kw), BPR(user, item, **kw)
    nu, ni, K = STEP["nu"], STEP["ni"], 5
    assert torch.equal(h.user_embeddings, b.user_factors) and torch.equal(h.item_embeddings, b.item_factors)
    start = _host_state(h)
    u, i, j, valid, _ = (t.cpu().numpy() for t in h.sample(K))
    assert all(torch.equal(x, y) for x, y in zip(h.sample(K), b.sample(K)))
    lh, lb = h.train_steps(K), b.train_steps(K)
    state, _ = _reference_steps(start, href.identity_bags(nu), href.identity_bags(ni), u, i, j, valid, h.reg, h.lr, "adagrad", K)
    got_h = _host_state(h)
    got_b = {"user": b.user_factors.cpu().numpy(), "item": b.item_factors.cpu().numpy(), "user_acc": b.user_accum.cpu().numpy(),
             "item_acc": b.item_accum.cpu().numpy()}
    bound = {}
    for key in ("user", "item", "user_acc", "item_acc"):
        _within("identity-%s" % key, got_h[key], state[np.float32][key], state[np.float64][key])
        e32 = bref.arr_err(state[np.float32][key], state[np.float64][key])
        bound[key] = href.FACTOR * e32 + href.FLOOR
        assert rel_err(got_b[key], state[np.float64][key]) <= bound[key], key
    same = all(np.array_equal(got_h[k], got_b[k]) for k in got_h) and lh == lb
    print("identity-only HybridBPR against BPR after %d steps: bit equality %s" % (K, same))
    _note("identity-bit-equal-to-bpr", bool(same))
    # auc: the two models' rows differ by at most twice the bound of their scale; d = x . (yi - yj) then moves by at most
    # 2 D S_u S_i (e_u + e_i), and only a triple whose |d| is below that can be ordered differently
    S_u, S_i = np.abs(got_b["user"]).max(), np.abs(got_b["item"]).max()
    move = 2 * STEP["rank"] * S_u * S_i * 2 * (bound["user"] + bound["item"])
    tu, ti, tj, tv, _ = b.sample(2, step0=0, seed=b.seed + 1)
    from esrecsys_amd import ops
    _, d, _ = ops.bpr_fwd_bwd(b.user_factors, b.item_factors, tu.reshape(-1), ti.reshape(-1), tj.reshape(-1), tv.reshape(-1),
                              0.0, want_grads=False, want_diff=True)
    ok = tv.reshape(-1) != 0
    near = int(((d.abs() <= move) & ok).sum())
    auc_h, auc_b = h.auc(K=2), b.auc(K=2)
    print("auc %.6f (hybrid) %.6f (bpr); %d of %d triples within %.3g of a tie" % (auc_h, auc_b, near, int(ok.sum()), move))
    assert abs(auc_h - auc_b) <= near / int(ok.sum())


def test_recommend_with_extra_items_equals_a_full_sort(dev):
    import torch
    m = _model(dev, "adagrad")
    m.train_steps(2)
    new_ids = np.array([5000, 260, 5001], np.int64)
    ids, rows = m.compose_items(np.repeat(new_ids, 2), np.array([7, 1003, 7, 2001, 1000, 7]), None)
    assert ids.tolist() == [260, 5000, 5001] and tuple(rows.shape) == (3, STEP["rank"])
    queries = np.array([0, 5, 119, 999], np.int64)                           # 999 is unknown
    k = 12
    rec, scores, lengths = (t.cpu().numpy() for t in m.recommend(queries, k=k, extra_items=(ids, rows)))
    X = m.user_rows().cpu().numpy().astype(np.float64)
    Y = torch.cat([m.item_rows(), rows]).cpu().numpy().astype(np.float64)
    all_ids = np.concatenate([m.items.cpu().numpy(), ids.cpu().numpy()]).astype(np.int64)
    user, item = _pairs(np.random.default_rng(21))
    assert lengths.tolist() == [k, k, k, 0] and (rec[3] == -1).all()
    for q, uid in enumerate(queries[:3]):
        s = (Y @ X[uid]).astype(np.float32)
        seen = set(item[user == uid].tolist())
        cand = sorted((-float(s[c]), int(all_ids[c])) for c in range(all_ids.size) if int(all_ids[c]) not in seen)[:k]
        assert rec[q].tolist() == [c[1] for c in cand], q
        assert np.max(np.abs(scores[q] + np.array([c[0] for c in cand]))) <= 1e-5
    # the extra items are never seen, and they can be recommended
    plain = m.recommend(queries, k=k)[0].cpu().numpy()
    assert not np.isin(plain, new_ids).any()
    with pytest.raises(ValueError, match="known item"):
        m.recommend(queries, k=k, extra_items=(torch.tensor([3]), rows[:1]))


def test_planted_corpus_cold_start(dev):
    """items of a cluster share a feature; a tenth of the items is in no pair; composed from their feature alone they reach
    the top k of their cluster's users far above chance (the fp64 restatement clears the same bar: test_hybrid_ref.py)"""
    from esrecsys_amd.factorization import HybridBPR
    P, c = href.PLANTED, href.planted()
    m = HybridBPR(c["user"], c["item"], item_features=(c["feat_item"], c["feat_id"], None), rank=P["rank"], batch=P["batch"],
                  reg=P["reg"], lr=P["lr"], seed=P["seed"], device=dev)
    before = m.auc(K=2)
    losses = m.fit(P["steps"])
    assert len(losses) == P["steps"] == m.step and np.isfinite(losses).all()
    assert np.mean(losses[-10:]) < np.mean(losses[:10]) and m.auc(K=2) > before
    extra = m.compose_items(c["new_item"], c["new_feat"])
    rec, _, lengths = m.recommend(np.arange(P["clusters"] * P["users_per"]), k=P["k"], extra_items=extra)
    assert int(lengths.min()) == P["k"]
    recall, chance = href.own_withheld_recall(rec.cpu().numpy(), c), href.planted_chance()
    print("hybrid planted corpus: loss %.4f -> %.4f, own withheld recall@%d %.3f, chance %.3f"
          % (np.mean(losses[:10]), np.mean(losses[-10:]), P["k"], recall, chance))
    _note("planted-recall-over-chance", recall / chance)
    assert recall > 5 * chance

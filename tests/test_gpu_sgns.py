"""GPU: skip-gram with negative sampling (esr_sgns.hip, factorization.SGNS) against tests/_sgns_ref.py -- the sampler bit for
bit, the forward / backward and the whole step under the rule of that module (kernel error against fp64 <= 4 e32 + 2^-22),
exactly representable tables bit for bit, one call past one grid, the failure bit, the model's neighbours and sequence
recommendations, and learning on the planted corpus against the fp64 fixture."""
import json
import os

import numpy as np
import pytest

import _sgns_ref as sref
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

NAMES = "c e o valid neg dropped".split()


def _t(dev, a, dt=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


@pytest.fixture(scope="module")
def corpus():
    """documents of the lengths (1, 2, 3, 5, 6, 33, 1000), ni = 1001, and the noise table of their counts"""
    return sref.boundary_corpus()


def _sample(dev, corpus, window, K, seed, step0, steps, B):
    from esrecsys_amd import ops
    (so, su, si), nd, ni, keep, alias = corpus
    out = ops.sgns_sample(_t(dev, so), _t(dev, su), _t(dev, si), nd, ni, window, K, _t(dev, keep.view(np.int32)), _t(dev, alias),
                          seed, step0, steps, B)
    return tuple(t.cpu().numpy() for t in out)


def _same_draw(got, want, what):
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, NAMES[n])


# ---- the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 5, 32])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_sampler_equals_the_restatement(dev, corpus, B, steps, window):
    (so, su, si), nd, ni, keep, alias = corpus
    assert tuple(np.diff(so)) == sref.DOC_LENGTHS and ni == 1001
    seed, step0 = (0xC0FFEE << 32) | 99, 2 ** 32 - 2                          # both key words; three steps wrap the step
    for K in (1, 5, 16):
        got = _sample(dev, corpus, window, K, seed, step0, steps, B)
        _same_draw(got, sref.sample_ref(so, su, si, nd, ni, window, K, keep, alias, seed, step0, steps, B), (B, steps, window, K))
        c, e, o, valid, neg, dropped = got
        assert np.array_equal(dropped, (valid == 0).sum(1))                   # dropped = the invalid slots
        doc = su[e]
        for k, t in zip(*np.nonzero(valid)):                                  # a valid (e, o): one document, within the window
            lo, hi = max(so[doc[k, t]], e[k, t] - window), min(so[doc[k, t] + 1], e[k, t] + window + 1)
            near = np.concatenate([si[lo:e[k, t]], si[e[k, t] + 1:hi]])
            assert o[k, t] in near and c[k, t] == si[e[k, t]]
        assert not valid[doc == 0].any()                                      # the document of length 1 only ever drops
        assert neg.shape == (steps, B, K) and neg.min() >= 0 and neg.max() < ni


def test_sampler_rows_and_prefixes_do_not_depend_on_the_launch(dev, corpus):
    three = _sample(dev, corpus, 5, 5, 5, 2 ** 32 - 2, 3, 257)
    for k in range(3):
        one = _sample(dev, corpus, 5, 5, 5, (2 ** 32 - 2 + k) % 2 ** 32, 1, 257)
        assert all(np.array_equal(a[k], b[0]) for a, b in zip(three, one)), k
    longer = _sample(dev, corpus, 5, 5, 5, 2 ** 32 - 2, 3, 300)
    assert all(np.array_equal(a, b[:, :257]) for a, b in zip(three[:5], longer[:5]))
    assert not np.array_equal(three[1][0], three[1][1]) and (three[5] > 0).all()
    more = _sample(dev, corpus, 5, 16, 5, 2 ** 32 - 2, 3, 257)                # the noise count enters neg alone
    assert all(np.array_equal(a, b) for a, b in zip(three[:4], more[:4])) and np.array_equal(three[4], more[4][:, :, :5])


# ---- forward / backward ----------------------------------------------------------------------------------------------------
def _tables(rng, ni, D):
    """rows of size D^(-1/4) per element: a score is of order 1"""
    s = D ** -0.25
    return tuple((rng.standard_normal((ni, D)) * s).astype(np.float32) for _ in range(2))


def _run(dev, tables, c, o, neg, valid, reg, **kw):
    import torch
    from esrecsys_amd import ops
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.sgns_fwd_bwd(*[_t(dev, a) for a in tables], _t(dev, c, np.int32), _t(dev, o, np.int32), _t(dev, neg, np.int32),
                           _t(dev, valid, np.int32), reg, failed=failed, **kw)
    return tuple(None if a is None else a.cpu().numpy() for a in out) + (int(failed.item()),)


def _parts(loss_t, s, grads, B, K):
    return {"loss_t": loss_t, "s": s, "centre": grads[:B], "positive": grads[B:2 * B], "noise": grads[2 * B:].reshape(K, B, -1)}


def _check_rule(got, tables, c, o, neg, valid, reg, what):
    r64, r32 = (sref.fwd_bwd_ref(*tables, c, o, neg, valid, reg, dt) for dt in (np.float64, np.float32))
    bound, e32 = sref.bounds(r32, r64, sref.KEYS)
    B, K = neg.shape
    assert got[2].shape == ((2 + K) * B, tables[0].shape[1]) and got[1].shape == (B, 1 + K)
    for k, g in _parts(*got[:3], B, K).items():
        assert np.isfinite(g).all(), (what, k)
        err = rel_err(g, r64[k])
        print("sgns_fwd_bwd %s %s: error %.3g  e32 %.3g  bound %.3g" % (what, k, err, e32[k], bound[k]))
        assert err <= bound[k], (what, k, err, e32[k], bound[k])


def _slots(rng, ni, B, K, tables):
    """B slots with the input condition of test_gpu_fpmc._slots for tiny batches: the errors are measured against the
    batch's largest value, so a batch of one or three slots takes the first draw whose fp64 |s_o| are all at least 1"""
    for _ in range(400):
        c, o, neg = rng.integers(0, ni, B), rng.integers(0, ni, B), rng.integers(0, ni, (B, K))
        if B > 3 or np.abs(sref.fwd_bwd_ref(*tables, c, o, neg, None, 0.0, np.float64)["s"][:, 0]).min() >= 1.0:
            return c, o, neg
    raise AssertionError("no draw keeps the input condition")


@pytest.mark.parametrize("B", [1, 3, 64, 257])
@pytest.mark.parametrize("D", [4, 8, 32, 64, 100, 128])
def test_fwd_bwd_against_fp64(dev, D, B):
    rng = np.random.default_rng([D, B])
    ni = 53
    tables = _tables(rng, ni, D)
    for K in (1, 5, 16):
        c, o, neg = _slots(rng, ni, B, K, tables)
        valid = np.ones(B, np.int32)
        if B >= 3:
            valid[1] = 0
            neg[2, K - 1] = o[2]                                              # n_k == o: skipped
        if B >= 64:
            neg[5:9, 0] = o[5:9]
            neg[10:13, :] = neg[10:13, :1]                                    # one noise id K times
            neg[13, :] = o[13]                                                # every noise item skipped
            c[14] = o[14]                                                     # the centre is its own context
        for reg in (0.0, 0.01):
            what = "D%d-B%d-K%d-reg%g" % (D, B, K, reg)
            got = _run(dev, tables, c, o, neg, valid, reg, want_diff=True)
            assert got[3] == 0
            _check_rule(got, tables, c, o, neg, valid, reg, what)
            loss_t, s, grads = got[:3]
            p = _parts(loss_t, s, grads, B, K)
            off = valid == 0
            assert not loss_t[off].any() and not s[off].any() and not p["centre"][off].any()        # exact zeros
            assert not p["positive"][off].any() and not p["noise"][:, off].any()
            if B >= 3:
                assert not p["noise"][K - 1, 2].any() and s[2, K] != 0                             # skipped, yet scored
            if B >= 64:
                assert not p["noise"][:, 13].any()
                assert np.array_equal(p["noise"][0, 10], p["noise"][K - 1, 10]) and (p["noise"][0, 10].any() or o[10] == neg[10, 0])
            # forward only, with and without the scores; no valid array: the valid slots keep their bits
            f = _run(dev, tables, c, o, neg, valid, reg, want_grads=False, want_diff=True)
            assert f[2] is None and np.array_equal(f[0], loss_t) and np.array_equal(f[1], s)
            n = _run(dev, tables, c, o, neg, valid, reg)
            assert n[1] is None and np.array_equal(n[0], loss_t) and np.array_equal(n[2], grads)
            a = _run(dev, tables, c, o, neg, None, reg, want_diff=True)
            keep = ~off
            assert np.array_equal(a[0][keep], loss_t[keep]) and np.array_equal(a[1][keep], s[keep]) and a[0].all()
            assert np.array_equal(a[2][np.tile(keep, 2 + K)], grads[np.tile(keep, 2 + K)])


@pytest.mark.parametrize("reg", [0.0, 0.25])
def test_exactly_representable_tables_are_bit_equal(dev, reg):
    """Entries are multiples of 1/4 in [-16, 16], D = 32 and reg a power of two: every product and sum of the scores and
    the rows is exact in float32 (|s| < 2^14 in steps of 2^-4), so the order of summation and the contraction of
    a * b + c do not show.  The sigmoids are exact too where the slots are kept: s = 0 gives 1 / 2 (centre row 0 is the
    zero vector), and |s| >= 128 gives expf(-|s|) = 0 -- below the smallest subnormal -- hence 0 or 1.  Only the loss
    (log1pf) is not exact."""
    rng = np.random.default_rng(5)
    ni, D, K = 30, 32, 5
    tables = tuple((rng.integers(-64, 65, (ni, D)) / 4.0).astype(np.float32) for _ in range(2))
    tables[0][0] = 0
    n = 6000
    c, o, neg = rng.integers(0, ni, n), rng.integers(0, ni, n), rng.integers(0, ni, (n, K))
    c[::5] = 0
    neg[::7, 2] = o[::7]
    s32 = sref.fwd_bwd_ref(*tables, c, o, neg, None, reg, np.float32)["s"]
    keep = ((s32 == 0) | (np.abs(s32) >= 128)).all(1)
    c, o, neg = c[keep], o[keep], neg[keep]
    B = c.size
    assert B >= 257 and (c == 0).sum() > 30 and (c != 0).sum() > 200 and (neg[:, 2] == o).sum() > 30
    valid = (np.arange(B) % 7 != 3).astype(np.int32)
    r32, r64 = (sref.fwd_bwd_ref(*tables, c, o, neg, valid, reg, dt) for dt in (np.float32, np.float64))
    assert np.array_equal(r32["s"], r64["s"])                                 # exact: float32 = fp64
    assert len(set(np.sign(r32["s"]).reshape(-1))) == 3 and r32["noise"].any()
    loss_t, s, grads, word = _run(dev, tables, c, o, neg, valid, reg, want_diff=True)
    assert word == 0 and np.array_equal(s, r32["s"]) and np.array_equal(grads, r32["grads"])
    assert rel_err(loss_t, r64["loss_t"]) <= sref.FLOOR


def test_one_call_past_one_grid_equals_two_calls_cut_at_an_odd_place(dev):
    """D = 4: one lane per slot, 256 slots per workgroup and a grid of at most 2048 workgroups (grid_for_groups, kMaxGrid)
    -- one pass serves 2048 * 256 = 524 288 slots, the last 257 are a second pass; the cut at 300 001 is no multiple of
    anything"""
    import torch
    from esrecsys_amd import ops
    rng = np.random.default_rng(9)
    ni, D, K, cut = 60, 4, 1, 300001
    B = 2048 * 256 + 257
    tables = [_t(dev, a) for a in _tables(rng, ni, D)]
    c, o = (_t(dev, rng.integers(0, ni, B), np.int32) for _ in range(2))
    neg = _t(dev, rng.integers(0, ni, (B, K)), np.int32)
    valid = _t(dev, rng.random(B) < 0.95, np.int32)
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    loss_t, s, grads = ops.sgns_fwd_bwd(*tables, c, o, neg, valid, 0.01, want_diff=True, failed=failed)
    parts = [ops.sgns_fwd_bwd(*tables, c[a:b], o[a:b], neg[a:b].contiguous(), valid[a:b], 0.01, want_diff=True, failed=failed)
             for a, b in ((0, cut), (cut, B))]
    assert int(failed.item()) == 0 and bool(loss_t[-257:].any())
    assert torch.equal(torch.cat([p[0] for p in parts]), loss_t) and torch.equal(torch.cat([p[1] for p in parts]), s)
    for r in range(2 + K):
        assert torch.equal(torch.cat([p[2][r * p[0].numel():(r + 1) * p[0].numel()] for p in parts]), grads[r * B:(r + 1) * B])


@pytest.mark.parametrize("D", [4, 100])
def test_ids_outside_the_tables_zero_their_slot_only(dev, D):
    from esrecsys_amd.factorization import FAIL_BAD_POSITION
    rng = np.random.default_rng(D)
    ni, B, K = 7, 70, 5
    tables = _tables(rng, ni, D)
    c, o, neg = _slots(rng, ni, B, K, tables)
    clean = _run(dev, tables, c, o, neg, None, 0.01, want_diff=True)
    assert clean[3] == 0
    for name, slot, value in (("c", 3, ni), ("o", 10, -1), ("neg", 20, ni), ("neg", 30, 2 ** 31 - 1), ("c", 40, -2 ** 31)):
        ids = dict(c=c.copy(), o=o.copy(), neg=neg.copy())
        if name == "neg":
            ids[name][slot, K - 1] = value
        else:
            ids[name][slot] = value
        valid = np.ones(B, np.int32)
        valid[slot] = slot % 20 != 0                                          # the bit is set whatever valid says
        got = _run(dev, tables, ids["c"], ids["o"], ids["neg"], valid, 0.01, want_diff=True)
        assert got[3] == FAIL_BAD_POSITION == 1 << 30, (name, slot)
        loss_t, s, grads = got[:3]
        assert not loss_t[slot] and not s[slot].any() and not grads[slot::B].any()
        others = np.arange(B) != slot
        assert np.array_equal(loss_t[others], clean[0][others]) and np.array_equal(s[others], clean[1][others])
        assert np.array_equal(grads[np.tile(others, 2 + K)], clean[2][np.tile(others, 2 + K)])


# ---- the step ----------------------------------------------------------------------------------------------------------------
STEP = dict(nd=60, ni=200, rank=8, batch=256, window=3, negatives=5)


def _zipf_documents(rng, nd, ni):
    p = 1.0 / np.arange(1, ni + 1) ** 1.1
    p /= p.sum()
    lengths = np.where(np.arange(nd) % 4 == 0, 1, rng.integers(2, 30, nd))      # every fourth document has one event
    doc = np.repeat(np.arange(nd), lengths)
    item = rng.choice(ni, doc.size, p=p)
    every = np.arange(ni)                                                    # and every item occurs somewhere
    return np.concatenate([doc, every % nd]), np.concatenate([item, every])


def _step_model(dev, optimizer, seed=4, **kw):
    from esrecsys_amd.factorization import SGNS
    doc, item = _zipf_documents(np.random.default_rng(21), STEP["nd"], STEP["ni"])
    return SGNS(doc, item, window=STEP["window"], negatives=STEP["negatives"], rank=STEP["rank"], batch=STEP["batch"],
                reg=sref.REG, optimizer=optimizer, seed=seed, device=dev, **kw)


def _state(m):
    return {k: getattr(m, k).cpu().numpy() for k in ("in_factors", "out_factors", "in_accum", "out_accum")}


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_three_steps_against_fp64(dev, optimizer):
    m = _step_model(dev, optimizer)
    nd, ni, B, K = STEP["nd"], STEP["ni"], STEP["batch"], STEP["negatives"]
    assert (m.users.numel(), m.items.numel()) == (nd, ni) and m.counts.sum() == m.n_events
    keep, alias = sref.alias_table(sref.noise_masses(m.counts.cpu().numpy()))
    assert np.array_equal(m.noise_keep.cpu().numpy().view(np.uint32), keep) and np.array_equal(m.noise_alias.cpu().numpy(), alias)
    start = _state(m)
    draw = tuple(t.cpu().numpy() for t in m.sample(3))
    so, su, si = m._seq_offsets, m._seq_upos.cpu().numpy(), m._seq_ipos.cpu().numpy()
    _same_draw(draw, sref.sample_ref(so, su, si, nd, ni, STEP["window"], K, keep, alias, m.seed, 0, 3, B), "step")
    c, _, o, valid, neg, dropped = draw
    assert len(np.unique(c)) < c.size // 4 and (valid == 0).any() and (neg == o[:, :, None]).any()
    losses = m.train_steps(3)
    assert m.step == 3 and len(losses) == 3
    state, ref_losses = {}, {}
    for dtype in (np.float64, np.float32):
        tables, accums, ref_losses[dtype] = [start["in_factors"], start["out_factors"]], [start["in_accum"], start["out_accum"]], []
        for k in range(3):
            r = sref.step_ref(tables, accums, c[k], o[k], neg[k], valid[k], m.reg, m.lr, optimizer, dtype)
            tables, accums = [r["in"], r["out"]], [r["in_acc"], r["out_acc"]]
            ref_losses[dtype].append(r["loss"])
        state[dtype] = {"in_factors": tables[0], "out_factors": tables[1], "in_accum": accums[0], "out_accum": accums[1]}
    keys = ("in_factors", "out_factors") + (("in_accum", "out_accum") if optimizer == "adagrad" else ())
    bound, e32 = sref.bounds(state[np.float32], state[np.float64], keys)
    now = _state(m)
    for key in keys:
        err = rel_err(now[key], state[np.float64][key])
        print("sgns step %s %s: error %.3g  e32 %.3g  bound %.3g x 3 steps" % (optimizer, key, err, e32[key], bound[key]))
        assert err <= 3 * bound[key], (key, err, e32[key], bound[key])
    for k in range(3):
        err = abs(losses[k] - ref_losses[np.float64][k]) / ref_losses[np.float64][k]
        print("sgns step %s loss %d: error %.3g" % (optimizer, k, err))
        assert err <= 1e-5, (k, err)
    # rows that no slot names keep their bits, tables and accumulators; the named ones moved
    named = {"in": c.reshape(-1), "out": np.concatenate([o.reshape(-1), neg.reshape(-1)])}
    for side in ("in", "out"):
        quiet = np.setdiff1d(np.arange(ni), named[side])
        assert quiet.size or side == "out", side                              # (768 x 6 context draws may name every item)
        assert np.array_equal(now[side + "_factors"][quiet], start[side + "_factors"][quiet])
        assert np.array_equal(now[side + "_accum"][quiet], start[side + "_accum"][quiet])
        rows = np.unique(named[side])
        assert not np.array_equal(now[side + "_factors"][rows], start[side + "_factors"][rows])
        if optimizer == "sgd":
            assert np.array_equal(now[side + "_accum"], start[side + "_accum"])


def test_train_steps_raise_on_a_position_outside_the_table(dev):
    from esrecsys_amd.factorization import FactorizationError
    m = _step_model(dev, "adagrad")
    m._seq_ipos[:] = STEP["ni"]                                               # every centre lies outside the tables
    with pytest.raises(FactorizationError, match="bit 30"):
        m.train_steps(1)
    with pytest.raises(FactorizationError, match="bit 30"):
        m.accuracy()


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_constructor_on_the_device(dev):
    import torch
    from esrecsys_amd.factorization import SGNS
    doc, item = [7, 7, 3, 7, 3, 7], [5, 9, 5, 5, 8, 5]                        # repeats are kept, in the order given
    m = SGNS(doc, item, window=2, negatives=3, rank=4, batch=8, seed=2, device=dev)
    assert m.items.tolist() == [5, 8, 9] and m.counts.tolist() == [4, 1, 1] and m.step == 0 and m.n_events == 6
    assert m._seq_offsets.tolist() == [0, 2, 6] and m._seq_ipos.tolist() == [0, 1, 0, 2, 0, 0]
    gen = torch.Generator(device="cpu").manual_seed(2)
    for table in (m.in_factors, m.out_factors):                               # in, then out
        assert torch.equal(table.cpu(), torch.randn(3, 4, generator=gen) * 0.5)
    t = SGNS(doc, item, time=[5.0, 1.0, 2.0, 1.0, 1.5, 0.5], window=2, rank=4, batch=8, device=dev)
    assert t._seq_ipos.tolist() == [1, 0, 0, 2, 0, 0]                         # a stable sort on (doc, time)
    d = SGNS.from_documents([7, 2, 7, 7, 5], [0, 3, 3, 5], window=1, negatives=2, rank=4, batch=8, device=dev)
    assert d.items.tolist() == [2, 5, 7] and d._seq_ipos.tolist() == [2, 0, 2, 2, 1]
    c, e, o, valid, neg, dropped = d.sample(3)
    assert tuple(c.shape) == (3, 8) and tuple(neg.shape) == (3, 8, 2) and tuple(dropped.shape) == (3,)
    losses = d.fit(2)
    assert len(losses) == 2 and d.step == 2 and 0.0 <= d.accuracy() <= 1.0
    for refused in (d.score, d.recommend, d.auc):
        with pytest.raises(TypeError, match="no user table"):
            refused([0])
    with pytest.raises(ValueError, match="which"):
        d.item_rows("both")


def _served_model(dev):
    from esrecsys_amd.factorization import SGNS
    rng = np.random.default_rng(31)
    lengths = rng.integers(1, 12, 30)
    doc = np.repeat(np.arange(30), lengths)
    item = rng.integers(0, 45, doc.size)
    m = SGNS(doc, item * 2, window=3, negatives=4, rank=8, batch=128, device=dev)     # ids are not positions
    m.train_steps(3)
    return m, item * 2


def _unit(rows):
    rows = rows.astype(np.float64)
    norm = np.sqrt((rows * rows).sum(1, keepdims=True))
    return np.where(norm > 0, rows / np.where(norm > 0, norm, 1.0), 0.0).astype(np.float32)


def test_similar_items(dev):
    import torch
    m, _ = _served_model(dev)
    m.in_factors[7] = m.in_factors[3]                                         # equal rows: ordered by item id
    items = m.items.cpu().numpy().astype(np.int64)
    unit = _unit(m.item_rows("in").cpu().numpy())
    assert np.array_equal(m.item_rows("in", normalize=True).cpu().numpy(), unit)
    assert torch.equal(m.item_rows("out"), m.out_factors)
    sim = (unit.astype(np.float64) @ unit.astype(np.float64).T).astype(np.float32)
    queries = np.array([items[0], items[3], 1, items[7], items[-1]], np.int64)      # 1 is no item
    for exclude in (True, False):
        ids, scores, lengths = (t.cpu().numpy() for t in m.similar_items(queries, k=6, exclude_self=exclude))
        for q, raw in enumerate(queries):
            if raw not in items:
                assert lengths[q] == 0 and (ids[q] == -1).all() and not scores[q].any()
                continue
            row = int(np.searchsorted(items, raw))
            order = sorted((-float(sim[row, n]), int(items[n])) for n in range(items.size) if not (exclude and n == row))[:6]
            assert lengths[q] == 6 and ids[q].tolist() == [v[1] for v in order], (q, exclude)
            assert np.allclose(scores[q], [-v[0] for v in order], rtol=0, atol=2.0 ** -20)
        if not exclude:
            assert ids[0, 0] == items[0] and ids[1, :2].tolist() == [items[3], items[7]]


def test_recommend_sequences(dev):
    import torch
    from esrecsys_amd import evaluate
    m, item = _served_model(dev)
    items = m.items.cpu().numpy().astype(np.int64)
    docs = [[item[0], 999, item[5], item[9], item[2]], [999], [], [item[3]], [item[4], item[4]]]      # 999 is no item: skipped
    ids = np.array([v for d in docs for v in d], np.int64)
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    V, W = m.in_factors.cpu().numpy().astype(np.float64), m.out_factors.cpu().numpy().astype(np.float64)
    rows = m.query_rows(ids, off).cpu().numpy()
    assert rows.shape == (5, 8) and not rows[1].any() and not rows[2].any()
    for exclude in (True, False):
        got = m.recommend_sequences(ids, off, k=5, exclude_seen=exclude)
        got_ids, got_scores, got_len = (t.cpu().numpy() for t in got)
        for q, doc in enumerate(docs):
            known = [int(np.searchsorted(items, v)) for v in doc if v in items]
            tail = known[-3:]
            mean = np.zeros(8, np.float32)
            for l in tail:                                                    # the chain of the bag rule, in float32
                mean = (mean.astype(np.float64) + np.float64(np.float32(1) / np.float32(len(tail))) * V[l]).astype(np.float32)
            assert np.allclose(rows[q], mean, rtol=0, atol=2.0 ** -22)
            score = (rows[q].astype(np.float64)[None, :] * W).sum(1)
            order = sorted((-float(np.float32(score[n])), int(items[n])) for n in range(items.size)
                           if not (exclude and n in known))[:5]
            assert got_len[q] == 5 and got_ids[q].tolist() == [v[1] for v in order], (q, exclude)
            assert np.allclose(got_scores[q], [-v[0] for v in order], rtol=0, atol=2.0 ** -20)
    truth = torch.tensor([int(items[1]), int(items[2]), int(items[3]), int(items[4]), int(items[5])], dtype=torch.int32)
    metrics = evaluate.ranking_metrics(got[0], got[2], truth, np.arange(6, dtype=np.int64), ks=(1, 5))
    assert metrics is not None
    div = m.diversify(*got, lam=1.0)
    assert torch.equal(div[0], got[0])                                        # lam = 1 keeps the order


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_planted_corpus_neighbours_follow_the_fp64_fixture(dev):
    from esrecsys_amd.factorization import SGNS
    P = sref.PLANTED
    fixture = json.load(open(os.path.join(GOLDEN, "sgns_planted.json")))
    assert fixture["settings"] == P and fixture["chance"] == 31.0 / 63.0
    bar = fixture["chance"] + 0.5 * (fixture["own_share_at_5"] - fixture["chance"])
    indices, offsets = sref.planted_documents()
    m = SGNS.from_documents(indices, offsets, window=P["window"], negatives=P["negatives"], rank=P["rank"], batch=P["batch"],
                            reg=0.0, lr=sref.LR, seed=P["seed"], device=dev)
    before = m.accuracy()
    losses = m.fit(P["steps"])
    assert np.isfinite(losses).all() and np.mean(losses[-10:]) < np.mean(losses[:10]) and m.accuracy() > before
    ids, _, lengths = m.similar_items(np.arange(P["ni"]), k=P["k"])
    assert int(lengths.min()) == P["k"]
    half = P["ni"] // 2
    share = float(((ids.cpu().numpy() >= half) == (np.arange(P["ni"]) >= half)[:, None]).mean())
    print("sgns planted corpus: own-community share@5 %.3f  fp64 restatement %.3f  (bar %.3f, chance %.3f)"
          % (share, fixture["own_share_at_5"], bar, fixture["chance"]))
    # the bar leaves half of the restatement's gain over chance for float32 against fp64 trajectories and the other start
    assert share >= bar, (share, bar)

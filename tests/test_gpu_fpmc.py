"""GPU: the Factorised Personalised Markov Chain (esr_fpmc.hip, factorization.FPMC) against tests/_fpmc_ref.py -- the
sampler bit for bit, the forward / backward and the whole step under the rule of that module (kernel error against fp64 <=
4 e32 + 2^-22), exactly representable tables bit for bit, one call past one grid, the refusals, the model's rows,
recommendations and sessions, and learning on the planted chain against BPR and the fp64 fixture."""
import json
import os

import numpy as np
import pytest

import _bpr_ref as bref
import _fpmc_ref as fref
from conftest import GOLDEN, rel_err

pytestmark = pytest.mark.gpu

SEQ_LENGTHS = (1, 2, 3, 4, 8, 9, 1000)
ROW_LENGTHS = (1, 2, 63, 64, 65, 1000, 3)            # the seen rows: around the binary search's boundaries
NAMES = "u e c i j valid dropped".split()


def _t(dev, a, dt=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


@pytest.fixture(scope="module")
def boundary_csrs():
    """sequences of every length around the window's boundaries and an independent seen CSR around the search's, ni = 1001"""
    rng = np.random.default_rng(11)
    (so, su, si), _ = fref.seq_csr({u: rng.integers(0, 1001, n).tolist() for u, n in enumerate(SEQ_LENGTHS)}, 7)
    ro, _, ri = bref.random_csr(rng, 7, 1001, ROW_LENGTHS)
    return (so, su, si, ro, ri), 7, 1001


def _sample(dev, csrs, nu, ni, window, seed, step0, K, B):
    from esrecsys_amd import ops
    so, su, si, ro, ri = csrs
    out = ops.fpmc_sample(_t(dev, so), _t(dev, su), _t(dev, si), _t(dev, ro), _t(dev, ri), nu, ni, window, seed, step0, K, B)
    return tuple(t.cpu().numpy() for t in out)


def _same_draw(got, want, what):
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, NAMES[n])


# ---- the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 3, 8])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_sampler_equals_the_restatement(dev, boundary_csrs, B, K, window):
    csrs, nu, ni = boundary_csrs
    seed, step0 = (0xC0FFEE << 32) | 99, 2 ** 32 - 2                          # both key words; K = 3 wraps the step
    got = _sample(dev, csrs, nu, ni, window, seed, step0, K, B)
    _same_draw(got, fref.sample_ref(*csrs, nu, ni, window, seed, step0, K, B), (B, K, window))
    assert np.array_equal(got[6], (got[5] == 0).sum(1))                       # dropped = the invalid slots
    so = csrs[0]
    assert (got[1] - got[2] >= so[got[0]]).all() and (got[2] <= window).all()  # no context crosses into the user before


def test_sampler_drops_and_short_sequences(dev):
    (so, su, si), (ro, ri) = fref.seq_csr({0: [0, 1, 2, 1], 1: [], 2: [2], 3: [0, 1]}, 4)
    got = _sample(dev, (so, su, si, ro, ri), 4, 3, 2, 3, 0, 2, 300)          # user 0 has seen all three items
    _same_draw(got, fref.sample_ref(so, su, si, ro, ri, 4, 3, 2, 3, 0, 2, 300), "drops")
    assert (got[5][got[0] == 0] == 0).all() and (got[0] == 0).any() and not (got[0] == 1).any()
    assert np.array_equal(got[6], (got[5] == 0).sum(1)) and got[6].sum() >= (got[0] == 0).sum()
    assert not got[2][got[0] == 2].any() and set(got[2][got[0] == 0]) == {0, 1, 2}


def test_sampler_rows_and_prefixes_do_not_depend_on_the_launch(dev, boundary_csrs):
    csrs, nu, ni = boundary_csrs
    three = _sample(dev, csrs, nu, ni, 3, 5, 2 ** 32 - 2, 3, 257)
    for k in range(3):
        one = _sample(dev, csrs, nu, ni, 3, 5, (2 ** 32 - 2 + k) % 2 ** 32, 1, 257)
        assert all(np.array_equal(a[k], b[0]) for a, b in zip(three, one)), k
    longer = _sample(dev, csrs, nu, ni, 3, 5, 2 ** 32 - 2, 3, 300)
    assert all(np.array_equal(a, b[:, :257]) for a, b in zip(three[:6], longer[:6]))
    assert not np.array_equal(three[1][0], three[1][1])


# ---- forward / backward ----------------------------------------------------------------------------------------------------
TABLE_KEYS = ("loss_t", "d", "five", "ctx")


def _tables(rng, nu, ni, D):
    """rows of size D^(-1/4) per element: both halves of d are of order 1"""
    s = D ** -0.25
    return tuple((rng.standard_normal((n, D)) * s).astype(np.float32) for n in (nu, ni, ni, ni))


def _run(dev, tables, seq, u, e, c, i, j, valid, reg, **kw):
    import torch
    from esrecsys_amd import ops
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.fpmc_fwd_bwd(*[_t(dev, a) for a in tables], _t(dev, seq, np.int32), *[_t(dev, a, np.int32) for a in (u, e, c, i, j)],
                           _t(dev, valid, np.int32), reg, failed=failed, **kw)
    return tuple(None if o is None else o.cpu().numpy() for o in out) + (int(failed.item()),)


def _ref(tables, seq, u, e, c, i, j, valid, reg, dtype):
    loss_t, d, grads, ids = fref.fwd_bwd_ref(*tables, seq, u, e, c, i, j, valid, reg, dtype)
    B = len(u)
    return {"loss_t": loss_t, "d": d, "five": grads[:5 * B], "ctx": grads[5 * B:], "ctx_ids": ids}


def _check_rule(got, tables, seq, u, e, c, i, j, valid, reg, what):
    r64, r32 = (_ref(tables, seq, u, e, c, i, j, valid, reg, dt) for dt in (np.float64, np.float32))
    bound, e32 = fref.bounds(r32, r64, TABLE_KEYS)
    B = len(u)
    loss_t, d, grads, ctx_ids = got[:4]
    assert grads.shape == (5 * B + int(np.sum(c)), tables[0].shape[1])
    assert ctx_ids.dtype == np.int32 and np.array_equal(ctx_ids, r64["ctx_ids"]), what
    for k, g in zip(TABLE_KEYS, (loss_t, d, grads[:5 * B], grads[5 * B:])):
        assert np.isfinite(g).all(), (what, k)
        err = rel_err(g, r64[k])
        print("fpmc_fwd_bwd %s %s: error %.3g  e32 %.3g  bound %.3g" % (what, k, err, e32[k], bound[k]))
        assert err <= bound[k], (what, k, err, e32[k], bound[k])


def _slots(rng, seq, nu, ni, B, window, tables):
    """B slots over `seq` with the input condition of the BPR test for tiny batches: the errors are measured against max |d|
    of the batch, so a batch of one or three slots takes the first draw whose fp64 |d| are all at least 1"""
    for _ in range(200):
        e = rng.integers(0, seq.size, B)
        c = np.minimum(e, window)
        u, i, j = rng.integers(0, nu, B), seq[e], rng.integers(0, ni, B)
        if B > 3 or np.abs(fref.fwd_bwd_ref(*tables, seq, u, e, c, i, j, None, 0.0, np.float64)[1]).min() >= 1.0:
            return u, e, c, i, j
    raise AssertionError("no draw keeps the input condition")


@pytest.mark.parametrize("B", [1, 3, 64, 257])
@pytest.mark.parametrize("D", [4, 8, 32, 64, 100, 128])
def test_fwd_bwd_against_fp64(dev, D, B):
    rng = np.random.default_rng([D, B])
    nu, ni = 37, 53
    tables = _tables(rng, nu, ni, D)
    seq = rng.integers(0, ni, 300)
    seq[100:109] = 7                                                          # a run of one item: repeated context items
    for window in (1, 3, 8):
        u, e, c, i, j = _slots(rng, seq, nu, ni, B, window, tables)
        valid = np.ones(B, np.int32)
        if B >= 3:
            valid[1] = 0                                                      # (its context rows keep their ids)
            e[1], c[1] = 50, window
        if B >= 64:
            j[5:9] = i[5:9]                                                   # i == j
            e[10:13], c[10:13] = (0, 1, 2), (0, 0, 0)                         # no context: the first event, and cut short
            e[13], c[13], i[13] = 108, window, 7                              # the context 7 .. 7, and i inside it
        for reg in (0.0, 0.01):
            what = "D%d-B%d-w%d-reg%g" % (D, B, window, reg)
            got = _run(dev, tables, seq, u, e, c, i, j, valid, reg, want_diff=True)
            assert got[4] == 0
            _check_rule(got, tables, seq, u, e, c, i, j, valid, reg, what)
            loss_t, d, grads, ctx_ids = got[:4]
            off = valid == 0
            assert not loss_t[off].any() and not d[off].any() and not grads[:5 * B][np.tile(off, 5)].any()    # exact zeros
            assert not grads[5 * B:][np.repeat(off, c)].any()
            if B >= 64:
                assert not grads[3 * B + 10:3 * B + 13].any() or reg > 0      # c = 0: the Bn rows are the L2 term alone
                assert np.array_equal(grads[3 * B + 10], np.float32(reg) * tables[2][i[10]])
                k0 = int(c[:13].sum())
                assert (ctx_ids[k0:k0 + window] == 7).all()
            # forward only, with and without the difference; no valid array: the valid slots keep their bits
            f = _run(dev, tables, seq, u, e, c, i, j, valid, reg, want_grads=False, want_diff=True)
            assert f[2] is None and f[3] is None and np.array_equal(f[0], loss_t) and np.array_equal(f[1], d)
            n = _run(dev, tables, seq, u, e, c, i, j, valid, reg)
            assert n[1] is None and np.array_equal(n[0], loss_t) and np.array_equal(n[2], grads)
            a = _run(dev, tables, seq, u, e, c, i, j, None, reg, want_diff=True)
            keep = ~off
            assert np.array_equal(a[0][keep], loss_t[keep]) and np.array_equal(a[1][keep], d[keep])
            assert np.array_equal(a[2][:5 * B][np.tile(keep, 5)], grads[:5 * B][np.tile(keep, 5)])
            assert np.array_equal(a[2][5 * B:][np.repeat(keep, c)], grads[5 * B:][np.repeat(keep, c)])
            assert np.array_equal(a[3], ctx_ids) and a[0].all()


@pytest.mark.parametrize("reg", [0.0, 0.25])
def test_exactly_representable_tables_are_bit_equal(dev, reg):
    """Entries are multiples of 1/4 in [-16, 16], D = 32, w = 1 / c with c in {1, 2, 4, 8} and reg a power of two: every
    product and sum of m, d and the rows is exact in float32 (|d| < 2^15 in steps of 2^-7), so the order of summation and
    the contraction of a * b + c do not show.  g is exact too where the slots are kept: d = 0 gives g = 1 / 2 (i == j), and
    |d| >= 128 gives expf(-|d|) = 0 -- below the smallest subnormal -- hence g = 0 or 1.  Only the loss (log1pf) is not
    exact."""
    rng = np.random.default_rng(5)
    nu, ni, D, window = 20, 30, 32, 8
    tables = tuple((rng.integers(-64, 65, (n, D)) / 4.0).astype(np.float32) for n in (nu, ni, ni, ni))
    seq = rng.integers(0, ni, 200)
    n = 600
    e = rng.integers(8, seq.size, n)
    c = np.array([1, 2, 4, 8])[np.arange(n) % 4]
    u, i, j = rng.integers(0, nu, n), seq[e], rng.integers(0, ni, n)
    j[::5] = i[::5]
    d32 = fref.fwd_bwd_ref(*tables, seq, u, e, c, i, j, None, reg, np.float32)[1]
    keep = (d32 == 0) | (np.abs(d32) >= 128)
    u, e, c, i, j = (a[keep] for a in (u, e, c, i, j))
    B = u.size
    assert B >= 257 and all((c == k).sum() > 30 for k in (1, 2, 4, 8))
    valid = (np.arange(B) % 7 != 3).astype(np.int32)
    r32 = _ref(tables, seq, u, e, c, i, j, valid, reg, np.float32)
    r64 = _ref(tables, seq, u, e, c, i, j, valid, reg, np.float64)
    assert np.array_equal(r32["d"], r64["d"])                                 # exact: float32 = fp64
    assert len(set(np.sign(r32["d"]))) == 3 and r32["ctx"].any()
    loss_t, d, grads, ctx_ids, word = _run(dev, tables, seq, u, e, c, i, j, valid, reg, want_diff=True)
    assert word == 0 and np.array_equal(ctx_ids, r32["ctx_ids"])
    assert np.array_equal(d, r32["d"]) and np.array_equal(grads[:5 * B], r32["five"]) and np.array_equal(grads[5 * B:], r32["ctx"])
    assert rel_err(loss_t, r64["loss_t"]) <= fref.FLOOR


def test_one_call_past_one_grid_equals_calls_of_257(dev):
    """D = 4: one lane per slot, 256 slots per workgroup and a grid of 2048 -- the last 257 slots are a second pass"""
    import torch
    from esrecsys_amd import ops
    rng = np.random.default_rng(9)
    nu, ni, D, step = 50, 60, 4, 257
    B = 2048 * 256 + step
    tables = [_t(dev, a) for a in _tables(rng, nu, ni, D)]
    seq = rng.integers(0, ni, 500)
    e = rng.integers(0, seq.size, B)
    c = np.minimum(e, 1)
    oo = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    seq_d, oo_d = _t(dev, seq, np.int32), _t(dev, oo)
    u, e_d, c_d, i, j = (_t(dev, a, np.int32) for a in (rng.integers(0, nu, B), e, c, seq[e], rng.integers(0, ni, B)))
    valid = _t(dev, rng.random(B) < 0.95, np.int32)
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    loss_t, d, grads, ctx_ids = ops.fpmc_fwd_bwd(*tables, seq_d, u, e_d, c_d, i, j, valid, 0.01, ctx_offsets=oo_d, M=int(oo[-1]),
                                                 want_diff=True, failed=failed)
    parts = []
    for a in range(0, B, step):
        b = min(a + step, B)
        parts.append(ops.fpmc_fwd_bwd(*tables, seq_d, u[a:b], e_d[a:b], c_d[a:b], i[a:b], j[a:b], valid[a:b], 0.01,
                                      ctx_offsets=(oo_d[a:b + 1] - oo_d[a]).contiguous(), M=int(oo[b] - oo[a]), want_diff=True,
                                      failed=failed))
    assert int(failed.item()) == 0 and len(parts) == 2041 + 1
    assert torch.equal(torch.cat([p[0] for p in parts]), loss_t) and torch.equal(torch.cat([p[1] for p in parts]), d)
    assert torch.equal(torch.cat([p[3] for p in parts]), ctx_ids) and bool(loss_t[-step:].any())
    for r in range(5):
        assert torch.equal(torch.cat([p[2][r * p[0].numel():(r + 1) * p[0].numel()] for p in parts]), grads[r * B:(r + 1) * B])
    assert torch.equal(torch.cat([p[2][5 * p[0].numel():] for p in parts]), grads[5 * B:])


@pytest.mark.parametrize("D", [4, 100])
def test_ids_outside_each_table_zero_their_slot_only(dev, D):
    from esrecsys_amd.factorization import FAIL_BAD_POSITION
    rng = np.random.default_rng(D)
    nu, ni, B, window = 6, 7, 70, 3
    tables = _tables(rng, nu, ni, D)
    seq = rng.integers(0, ni, 90)
    u, e, c, i, j = _slots(rng, seq, nu, ni, B, window, tables)
    e[:] = np.maximum(e, 10)
    c[:] = window
    i = seq[e]
    clean = _run(dev, tables, seq, u, e, c, i, j, None, 0.01, want_diff=True)
    assert clean[4] == 0
    bad_seq = seq.copy()
    bad_seq[5] = ni                                                           # the P table: a context id outside it
    cases = {"U": ("u", 3, nu), "A": ("i", 10, ni), "Bn": ("j", 20, -1), "P": ("e", 30, 7), "U-top": ("u", 40, 2 ** 31 - 1)}
    for table, (name, slot, value) in cases.items():
        ids = dict(u=u.copy(), e=e.copy(), c=c.copy(), i=i.copy(), j=j.copy())
        ids[name][slot] = value
        got = _run(dev, tables, bad_seq, *[ids[k] for k in "uecij"], None, 0.01, want_diff=True)
        assert got[4] == FAIL_BAD_POSITION == 1 << 30, table
        _check_rule(got, tables, bad_seq, *[ids[k] for k in "uecij"], None, 0.01, "bad-%s-D%d" % (table, D))
        loss_t, d, grads, ctx_ids = got[:4]
        assert not loss_t[slot] and not d[slot] and not grads[slot::B][:5].any() and not grads[5 * B + 3 * slot:][:3].any()
        others = np.arange(B) != slot
        assert np.array_equal(loss_t[others], clean[0][others]) and np.array_equal(d[others], clean[1][others])
        assert np.array_equal(grads[:5 * B][np.tile(others, 5)], clean[2][:5 * B][np.tile(others, 5)])
        assert np.array_equal(grads[5 * B:][np.repeat(others, 3)], clean[2][5 * B:][np.repeat(others, 3)])
        want_ids = clean[3].copy()
        if table == "P":
            want_ids[3 * slot:3 * slot + 3] = [bad_seq[4], 0, bad_seq[6]]       # events 4, 5, 6: the refused id reads as 0
        assert np.array_equal(ctx_ids, want_ids), table


# ---- the step ----------------------------------------------------------------------------------------------------------------
STEP = dict(nu=150, ni=200, rank=16, batch=257, window=3)


def _zipf_sequences(rng, nu, ni):
    p = 1.0 / np.arange(1, ni + 1) ** 1.1
    p /= p.sum()
    lengths = np.where(np.arange(nu) % 2 == 0, 1, rng.integers(2, 40, nu))      # every other user has one event
    user = np.repeat(np.arange(nu), lengths)
    item = rng.choice(ni, user.size, p=p)
    every = np.arange(ni)                                                    # and every item occurs somewhere
    return np.concatenate([user, every % nu]), np.concatenate([item, every])


def _step_model(dev, optimizer, seed=4, **kw):
    from esrecsys_amd.factorization import FPMC
    user, item = _zipf_sequences(np.random.default_rng(21), STEP["nu"], STEP["ni"])
    return FPMC(user, item, window=STEP["window"], rank=STEP["rank"], batch=STEP["batch"], optimizer=optimizer, seed=seed,
                device=dev, **kw)


def _state(m):
    return ({k: getattr(m, k + "_factors").cpu().numpy() for k in fref.TABLES},
            {k: getattr(m, k + "_accum").cpu().numpy() for k in fref.TABLES})


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_three_steps_against_fp64(dev, optimizer):
    m = _step_model(dev, optimizer)
    nu, ni, B = STEP["nu"], STEP["ni"], STEP["batch"]
    assert (m.users.numel(), m.items.numel()) == (nu, ni)
    start_t, start_a = _state(m)
    draw = tuple(t.cpu().numpy() for t in m.sample(3))
    so, su, si = m._seq_offsets, m._seq_upos.cpu().numpy(), m._seq_ipos.cpu().numpy()
    csrs = (so, su, si, m._user_offsets, m._row_ipos.cpu().numpy())
    _same_draw(draw, fref.sample_ref(*csrs, nu, ni, STEP["window"], m.seed, 0, 3, B), "step")
    assert len(np.unique(draw[3])) < draw[3].size // 4 and (draw[2] == 0).any() and (draw[2] == 3).any()
    losses = m.train_steps(3)
    assert m.step == 3 and len(losses) == 3
    state, ref_losses = {}, {}
    for dtype in (np.float64, np.float32):
        tables, accums, ref_losses[dtype] = dict(start_t), dict(start_a), []
        for k in range(3):
            r = fref.step_ref(tables, accums, si, *[a[k] for a in draw[:6]], m.reg, m.lr, optimizer, dtype)
            tables = {key: r[key] for key in fref.TABLES}
            accums = {key: r[key + "_acc"] for key in fref.TABLES}
            ref_losses[dtype].append(r["loss"])
        state[dtype] = dict(tables, **{k + "_acc": v for k, v in accums.items()})
    keys = fref.TABLES + (tuple(k + "_acc" for k in fref.TABLES) if optimizer == "adagrad" else ())
    bound, e32 = fref.bounds(state[np.float32], state[np.float64], keys)
    now_t, now_a = _state(m)
    got = dict(now_t, **{k + "_acc": v for k, v in now_a.items()})
    for key in keys:
        err = rel_err(got[key], state[np.float64][key])
        print("fpmc step %s %s: error %.3g  e32 %.3g  bound %.3g" % (optimizer, key, err, e32[key], bound[key]))
        assert err <= bound[key], (key, err, e32[key], bound[key])
    for k in range(3):
        e = abs(ref_losses[np.float32][k] - ref_losses[np.float64][k]) / ref_losses[np.float64][k]
        err = abs(losses[k] - ref_losses[np.float64][k]) / ref_losses[np.float64][k]
        print("fpmc step %s loss %d: error %.3g  e32 %.3g" % (optimizer, k, err, e))
        assert err <= fref.FACTOR * e + fref.FLOOR, (k, err, e)
    # rows that no slot names keep their bits, tables and accumulators; the named ones moved
    L, mask = fref.context_ids(si, draw[1].reshape(-1), draw[2].reshape(-1))
    named = {"user": draw[0], "item": np.concatenate([draw[3], draw[4]]), "next": np.concatenate([draw[3], draw[4]]),
             "prev": L[mask]}
    for key in fref.TABLES:
        quiet = np.setdiff1d(np.arange(nu if key == "user" else ni), named[key])
        assert quiet.size or key in ("item", "next"), key
        assert np.array_equal(now_t[key][quiet], start_t[key][quiet]) and np.array_equal(now_a[key][quiet], start_a[key][quiet])
        rows = np.unique(named[key])
        assert not np.array_equal(now_t[key][rows], start_t[key][rows])
        if optimizer == "sgd":
            assert np.array_equal(now_a[key], start_a[key])
    assert np.setdiff1d(np.arange(ni), named["prev"]).size > 0


def test_train_steps_raise_on_a_position_outside_the_table(dev):
    from esrecsys_amd.factorization import FactorizationError
    m = _step_model(dev, "adagrad")
    m._seq_ipos[:] = STEP["ni"]                                               # every context id lies outside P
    with pytest.raises(FactorizationError, match="bit 30"):
        m.train_steps(1)
    with pytest.raises(FactorizationError, match="bit 30"):
        m.auc()


# ---- the model -----------------------------------------------------------------------------------------------------------------
def test_constructor_on_the_device(dev):
    import torch
    from esrecsys_amd.factorization import FPMC
    for window in (0, 9):
        with pytest.raises(ValueError, match="window"):
            FPMC([0, 1], [0, 1], window=window, rank=4, device=dev)
    for rank in (2, 6, 132):
        with pytest.raises(ValueError, match="rank"):
            FPMC([0, 1], [0, 1], rank=rank, device=dev)
    with pytest.raises(ValueError, match="one length"):
        FPMC([0, 1], [0, 1], time=[1, 2, 3], rank=4, device=dev)
    user, item = [7, 7, 3, 7, 3, 7], [5, 9, 5, 5, 8, 5]                       # repeats are kept, in the order given
    m = FPMC(user, item, window=2, rank=4, batch=8, seed=2, device=dev)
    assert m.users.tolist() == [3, 7] and m.items.tolist() == [5, 8, 9] and m.step == 0 and m.n_events == 6 and m.nnz == 4
    assert m._seq_offsets.tolist() == [0, 2, 6] and m._seq_upos.tolist() == [0, 0, 1, 1, 1, 1]
    assert m._seq_ipos.tolist() == [0, 1, 0, 2, 0, 0] and m._row_ipos.tolist() == [0, 1, 0, 2]
    gen = torch.Generator(device="cpu").manual_seed(2)
    for table, n in ((m.user_factors, 2), (m.item_factors, 3), (m.next_factors, 3), (m.prev_factors, 3)):   # U, A, Bn, P
        assert torch.equal(table.cpu(), torch.randn(n, 4, generator=gen) * 0.5)
    # time: a stable sort on (user, time) -- equal times keep the order given
    time = [5.0, 1.0, 2.0, 1.0, 1.5, 0.5]
    t = FPMC(user, item, time=time, window=2, rank=4, batch=8, seed=2, device=dev)
    assert t._seq_ipos.tolist() == [1, 0, 0, 2, 0, 0] and t._seq_upos.tolist() == m._seq_upos.tolist()      # 9 before the 5 at 1.0
    order = sorted(range(6), key=lambda n: (user[n], time[n]))               # (sorted is stable)
    assert t._seq_ipos.tolist() == [m.items.tolist().index(item[n]) for n in order]
    assert FPMC(user, item, time=[3] * 6, window=2, rank=4, device=dev)._seq_ipos.tolist() == m._seq_ipos.tolist()
    d = FPMC.from_documents([7, 2, 7, 7, 5], [0, 3, 3, 5], window=1, rank=4, batch=8, device=dev)
    assert d.users.tolist() == [0, 2] and d.items.tolist() == [2, 5, 7] and d._seq_ipos.tolist() == [2, 0, 2, 2, 1]
    u, e, c, i, j, valid, dropped = d.sample(3)
    assert tuple(u.shape) == (3, 8) and tuple(dropped.shape) == (3,) and int(c.max()) <= 1
    losses = d.train_steps(2)
    assert len(losses) == 2 and d.step == 2 and 0.0 <= d.auc() <= 1.0


def _served_model(dev):
    from esrecsys_amd.factorization import FPMC
    rng = np.random.default_rng(31)
    lengths = rng.integers(1, 12, 30)
    user = np.repeat(np.arange(30), lengths)
    item = rng.integers(0, 45, user.size)
    m = FPMC(user * 3 + 1, item * 2, window=3, rank=8, batch=128, device=dev)  # ids are not positions
    m.train_steps(3)
    return m, user * 3 + 1, item * 2


def test_rows_scores_and_recommendations(dev):
    import torch
    from esrecsys_amd import ops
    m, user, item = _served_model(dev)
    nu, ni = m.users.numel(), m.items.numel()
    m.item_factors[7], m.next_factors[7] = m.item_factors[3], m.next_factors[3]      # equal rows: ordered by item id
    # query_rows = [U ; bag_sum(tail)] bit for bit, the bag built here from the sequences
    so, si = m._seq_offsets, m._seq_ipos.cpu().numpy()
    tails = [si[max(so[u], so[u + 1] - 3):so[u + 1]] for u in range(nu)]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tails])]).astype(np.int64)
    weight = np.concatenate([np.full(len(t), np.float32(1) / np.float32(len(t)), np.float32) for t in tails])
    bag = ops.bag_sum(m.prev_factors, _t(dev, off), _t(dev, np.concatenate(tails), np.int32), _t(dev, weight))
    rows = m.query_rows()
    assert rows.shape == (nu, 16) and torch.equal(rows, torch.cat([m.user_factors, bag], 1))
    assert torch.equal(m.item_rows(), torch.cat([m.item_factors, m.next_factors], 1))
    some = m.query_rows([4, 2, 1])                                            # 2 is unknown
    assert torch.equal(some[0], rows[1]) and torch.equal(some[2], rows[0]) and bool(some[1].isnan().all())
    # score = als_predict on those rows
    queries = np.array([1, 4, 2, 88, 1000, 4], np.int64)                      # 2 and 1000 are unknown
    items = m.items.cpu().numpy().astype(np.int64)
    flat = m.score(np.repeat(queries, ni), np.tile(items, queries.size))
    upos = m._positions(np.repeat(queries, ni), m.users)
    ipos = m._positions(np.tile(items, queries.size), m.items)
    assert torch.equal(flat.isnan(), upos < 0) and torch.equal(flat[upos >= 0],
                                                              ops.als_predict(rows, m.item_rows(), upos, ipos)[upos >= 0])
    table = flat.cpu().numpy().reshape(queries.size, ni)
    seen = set(zip(user.tolist(), item.tolist()))
    k = 10
    for exclude in (True, False):
        ids, scores, lengths = (t.cpu().numpy() for t in m.recommend(queries, k=k, exclude_seen=exclude))
        for q, uid in enumerate(queries):
            if uid not in m.users.tolist():
                assert lengths[q] == 0 and (ids[q] == -1).all() and not scores[q].any() and np.isnan(table[q]).all()
                continue
            cand = [(-table[q, c], int(items[c])) for c in range(ni) if not (exclude and (uid, int(items[c])) in seen)]
            order = sorted(cand)[:k]
            assert lengths[q] == len(order) == k and ids[q].tolist() == [c[1] for c in order], (q, exclude)
            assert scores[q].view(np.int32).tolist() == np.array([-c[0] for c in order], np.float32).view(np.int32).tolist()
    div = m.diversify(*m.recommend(queries, k=k), lam=1.0)
    assert torch.equal(div[0], m.recommend(queries, k=k)[0])                  # lam = 1 keeps the order


def test_recommend_sequences(dev):
    import torch
    m, user, item = _served_model(dev)
    items = m.items.cpu().numpy().astype(np.int64)
    # sessions of nobody: a brute-force ranking of m . Bn; 999 is no item and is skipped
    docs = [[item[0], 999, item[5], item[9], item[2]], [999], [], [item[3]], [item[4], item[4]]]
    ids = np.array([v for d in docs for v in d], np.int64)
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    P, Bn = m.prev_factors.cpu().numpy().astype(np.float64), m.next_factors.cpu().numpy().astype(np.float64)
    for exclude in (True, False):
        got_ids, got_scores, got_len = (t.cpu().numpy() for t in m.recommend_sequences(ids, off, k=5, exclude_seen=exclude))
        for q, doc in enumerate(docs):
            known = [int(np.searchsorted(items, v)) for v in doc if v in items]
            tail = known[-3:]
            mm = np.zeros(8, np.float32)
            for l in tail:                                                    # the chain of the bag rule, in float32
                mm = (mm.astype(np.float64) + np.float64(np.float32(1) / np.float32(len(tail))) * P[l]).astype(np.float32)
            score = (mm.astype(np.float64)[None, :] * Bn).sum(1)
            cand = [(-float(np.float32(score[c])), int(items[c])) for c in range(items.size)
                    if not (exclude and c in known)]
            order = sorted(cand)[:5]
            assert got_len[q] == 5 and got_ids[q].tolist() == [c[1] for c in order], (q, exclude)
            assert np.allclose(got_scores[q], [-c[0] for c in order], rtol=0, atol=2.0 ** -20)
    # a known user's own training sequence: recommend's lists
    users = m.users.cpu().numpy().astype(np.int64)[[0, 5, 17]]
    seqs = [item[user == u] for u in users]
    ids, off = np.concatenate(seqs), np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    for exclude in (True, False):
        a = m.recommend_sequences(ids, off, k=7, users=users, exclude_seen=exclude)
        b = m.recommend(users, k=7, exclude_seen=exclude)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), exclude


def test_split_last_equals_the_restatement(dev):
    import torch
    from esrecsys_amd import evaluate
    rng = np.random.default_rng(3)
    lengths = np.array([0, 1, 2, 3, 4, 2, 9, 3, 1, 30])
    ids = rng.integers(0, 50, lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)])
    for n_last, min_length in ((1, 3), (2, 3), (1, 2), (3, 9)):
        want = fref.split_last_ref(ids, off, n_last, min_length)
        for where in (None, dev):
            a = (ids, off) if where is None else (torch.from_numpy(ids).to(dev), torch.from_numpy(off).to(dev))
            got = evaluate.split_last(*a, n_last=n_last, min_length=min_length)
            assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want)), (n_last, min_length)
            assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_planted_chain_fpmc_beats_bpr_and_follows_the_fp64_fixture(dev):
    from esrecsys_amd import evaluate
    from esrecsys_amd.factorization import BPR, FPMC
    P = fref.PLANTED
    fixture = json.load(open(os.path.join(GOLDEN, "fpmc_planted.json")))
    assert {k: fixture["settings"][k] for k in P} == P
    indices, offsets = fref.planted_sequences()
    train, train_off, truth, truth_off, kept = evaluate.split_last(indices, offsets)
    assert kept.numel() == P["nu"]
    kw = dict(rank=P["rank"], batch=P["batch"], reg=fref.REG, lr=fref.LR, seed=P["seed"], device=dev)
    users = np.arange(P["nu"])
    rates = {}
    for name, model in (("fpmc", FPMC.from_documents(train, train_off, window=P["window"], **kw)),
                        ("bpr", BPR.from_documents(train, train_off, **kw))):
        losses = model.fit(P["steps"])
        assert np.isfinite(losses).all() and np.mean(losses[-10:]) < np.mean(losses[:10])
        ids, _, lengths = model.recommend(users, k=P["k"], exclude_seen=False)      # every item is a candidate, as in the fixture
        assert int(lengths.min()) == P["k"]
        rates[name] = float((ids.cpu().numpy() == truth.numpy()[:, None]).any(1).mean())
    mid = 0.5 * (rates["bpr"] + fixture["hit_rate_at_10"])
    print("fpmc planted chain: hit rate@10  fpmc %.3f  bpr %.3f  fp64 restatement %.3f  (midpoint %.3f, chance %.3f)"
          % (rates["fpmc"], rates["bpr"], fixture["hit_rate_at_10"], mid, fixture["chance"]))
    # the midpoint leaves half the measured gap for float32 trajectories, the tables' other random start and Adagrad's order
    assert rates["fpmc"] >= mid, (rates, mid)

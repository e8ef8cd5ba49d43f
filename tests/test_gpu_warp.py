"""GPU: the fused WARP step (esr_warp.hip, ops.warp_step, factorization.WARP) against tests/_warp_ref.py -- bit for bit on
the exact tables, selection on every decided slot and values under the rule of that module (kernel error against fp64
<= 4 e32 + 2^-22) on the random ones, independence of the launch, agreement with BPR's sampler, the error paths, and the
model end to end: its steps composed by hand, one step against fp64, its state, recommendations and learning."""
import numpy as np
import pytest

import _bpr_ref as bref
import _warp_ref as wref

pytestmark = pytest.mark.gpu


def _t(dev, a, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _run(dev, case, B=None, **kw):
    """ops.warp_step on a case of _warp_ref: a dict of numpy arrays and the failed word"""
    import torch
    from esrecsys_amd import ops
    off, upos, ipos = case["csr"]
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    kw.setdefault("want_diff", True)
    out = ops.warp_step(_t(dev, case["user"]), _t(dev, case["item"]), _t(dev, off, np.int64), _t(dev, upos, np.int32),
                        _t(dev, ipos, np.int32), _t(dev, case["weight"], np.float32), case["seed"], case["step"],
                        case["B"] if B is None else B, case["T"], float(case["margin"]), float(case["reg"]), failed=failed, **kw)
    got = dict(zip(wref.IDS + ("loss_t", "d", "grads"), (None if o is None else o.cpu().numpy() for o in out)))
    got["failed"] = int(failed.item())
    return got


def _same_bits(got, r, what):
    for k in wref.IDS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], r[k]), (what, k)
    for k in wref.ARRAYS:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], r[k].astype(np.float32)), (what, k)
    assert got["failed"] == 0


# ---- exact tables: bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", wref.EXACT_D)
def test_exact_grid_bit_for_bit(dev, D):
    mine = [(c, r) for c, r in wref.exact_cases() if c["name"].startswith("grid-D%d-" % D)]
    assert len(mine) == len(wref.EXACT_B) * len(wref.EXACT_T)
    for case, r in mine:
        _same_bits(_run(dev, case), r, case["name"])


def test_exact_planted_cases_bit_for_bit(dev):
    planted = {c["name"]: (c, r) for c, r in wref.exact_cases() if not c["name"].startswith("grid-")}
    assert set(planted) == {"seen-everything", "all-but-one", "one-item", "ties", "one-violator"}
    for name, (case, r) in planted.items():
        _same_bits(_run(dev, case), r, name)
    r = planted["seen-everything"][1]
    assert ((r["u"] == 0) <= ((r["valid"] == 0) & (r["trials"] == 0))).all() and (r["u"] == 0).any()
    assert not planted["one-item"][1]["valid"].any() and not planted["one-item"][1]["trials"].any()
    r = planted["all-but-one"][1]
    assert r["valid"].any() and (r["j"][r["valid"] == 1] == 77).all() and set(r["trials"].tolist()) == {0, 1}
    r = planted["ties"][1]
    assert r["valid"].all() and (r["j"] >= 30).all() and (r["d"] == 0.75 - 2.0 ** -6).all() and (r["trials"] > 1).any()
    r = planted["one-violator"][1]
    first_wave = r["trials"][:64]                                               # D = 64: four slots a wave
    assert (r["j"][r["valid"] == 1] == 40).all() and first_wave.min() <= 2 and first_wave.max() == 16


# ---- random tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(6))
def test_random_tables_selection_and_values(dev, n):
    case, r64, r32 = wref.random_cases()[n]
    got = _run(dev, case)
    assert got["failed"] == 0
    share = float(r64["undecided"].mean())
    assert share <= wref.UNDECIDED_CAP, (case["name"], share)
    same = wref.same_selection(got, r64)
    assert not (~same & ~r64["undecided"]).any(), (case["name"], np.flatnonzero(~same))
    agree = same & wref.same_selection(r32, r64)
    assert agree.mean() >= 1 - 2 * wref.UNDECIDED_CAP
    bound, e32 = wref.bounds(wref.restrict(r32, agree), wref.restrict(r64, agree), wref.ARRAYS)
    g, want = wref.restrict(got, agree), wref.restrict(r64, agree)
    for k in wref.ARRAYS:
        assert np.isfinite(got[k]).all(), (case["name"], k)
        err = wref.arr_err(g[k], want[k])
        print("warp_step %s %s: error %.3g  e32 %.3g  bound %.3g" % (case["name"], k, err, e32[k], bound[k]))
        assert err <= bound[k], (case["name"], k, err, e32[k], bound[k])
    off = got["valid"] == 0
    assert not got["loss_t"][off].any() and not got["d"][off].any() and not got["grads"][wref.slot_rows(off)].any()


# ---- independence of the launch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_prefixes_and_forward_only_calls_keep_their_bits(dev, n):
    case = wref.random_case_list()[n]
    B, D = 257, case["user"].shape[1]
    full = _run(dev, case, B=B)
    for Bp in (1, 63, 65):
        part = _run(dev, case, B=Bp)
        for k in wref.IDS + ("loss_t", "d"):
            assert np.array_equal(part[k], full[k][:Bp]), (Bp, k)
        assert np.array_equal(part["grads"].reshape(3, Bp, D), full["grads"].reshape(3, B, D)[:, :Bp]), Bp
    fwd = _run(dev, case, B=B, want_grads=False)
    assert fwd["grads"] is None and all(np.array_equal(fwd[k], full[k]) for k in wref.IDS + ("loss_t", "d"))
    bare = _run(dev, case, B=B, want_grads=False, want_diff=False)
    assert bare["d"] is None and all(np.array_equal(bare[k], full[k]) for k in wref.IDS + ("loss_t",))


# ---- agreement with BPR ----------------------------------------------------------------------------------------------------------
def test_where_every_unseen_candidate_violates_the_triples_are_bprs(dev):
    from esrecsys_amd import ops
    rng = np.random.default_rng(31)
    for nu, ni, lengths, B in ((9, 1001, (1, 2, 63, 64, 65, 1000), 257), (40, 12, (0, 1, 11, 12), 300), (2, 1, (1, 0), 65)):
        csr = bref.random_csr(rng, nu, ni, lengths)
        U, Y = wref.random_tables(rng, nu, ni, 8)
        case = wref._case("bpr", U, Y, csr, wref.harmonic(ni), (0xC0FFEE << 32) | 99, 2 ** 32 - 1, B, 15, 3e38, 0.0)
        got = _run(dev, case)
        u, i, j, valid, _ = ops.bpr_sample(_t(dev, csr[0], np.int64), _t(dev, csr[1], np.int32), _t(dev, csr[2], np.int32), nu, ni,
                                           case["seed"], case["step"], 1, B)
        for k, want in zip(("u", "i", "j", "valid"), (u, i, j, valid)):
            assert np.array_equal(got[k], want[0].cpu().numpy()), (nu, ni, k)
        assert np.array_equal(got["trials"], got["valid"]) and got["failed"] == 0


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def test_a_position_outside_the_table_sets_bit_30_and_writes_zeros(dev):
    rng = np.random.default_rng(32)
    U, Y = wref.random_tables(rng, 3, 9, 8)
    for bad_item in (9, 2 ** 31 - 1, -1):
        csr = (np.array([0, 1, 2, 3]), np.array([0, 1, 2]), np.array([4, bad_item, 5]))
        case = wref._case("bad", U, Y, csr, wref.harmonic(9), 3, 0, 257, 8, 1.0, 0.01)
        got, r = _run(dev, case), wref.reference(case, np.float64)
        assert got["failed"] == 1 << 30 and r["bad"]
        hit = got["i"] == bad_item
        assert hit.any() and not hit.all()
        for k in ("j", "valid", "trials", "loss_t", "d"):
            assert not got[k][hit].any(), k
        assert not got["grads"][wref.slot_rows(hit)].any()
        same = wref.same_selection(got, r)
        assert same[hit].all() and same.mean() > 0.9


def test_large_scores_stay_finite(dev):
    rng = np.random.default_rng(33)
    U, Y = wref.random_tables(rng, 5, 40, 32)
    case = wref._case("large", (U * 1e15).astype(np.float32), (Y * 1e15).astype(np.float32), bref.random_csr(rng, 5, 40, (3, 7)),
                      wref.harmonic(40), 4, 0, 257, 8, 1.0, 0.0)
    got = _run(dev, case)
    assert got["failed"] == 0 and got["valid"].any() and np.abs(got["d"]).max() > 1e29
    for k in wref.ARRAYS:
        assert np.isfinite(got[k]).all(), k
    r64 = wref.reference(case, np.float64)
    assert wref.same_selection(got, r64).mean() > 0.98


# ---- the model end to end ------------------------------------------------------------------------------------------------------
def _pairs(rng, nu=50, ni=70, n=600):
    return rng.integers(0, nu, n) * 3 + 1, rng.integers(0, ni, n) * 2          # sparse ids, repeated events


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_train_steps_equal_the_calls_composed_by_hand(dev, optimizer):
    import torch
    from esrecsys_amd import ops
    from esrecsys_amd.factorization import WARP
    user, item = _pairs(np.random.default_rng(41))
    kw = dict(rank=12, batch=300, seed=5, optimizer=optimizer, max_trials=8, margin=0.5, rank_weight="log1p", device=dev)
    a, b = WARP(user, item, **kw), WARP(user, item, **kw)
    losses = a.train_steps(3)
    nu, ni = b.users.numel(), b.items.numel()
    want_loss, want_trials = [], []
    for k in range(3):
        u, i, j, valid, trials, loss_t, _, grads = ops.warp_step(b.user_factors, b.item_factors, b._offsets_dev, b._row_upos,
                                                                 b._row_ipos, b.rank_weight, 5, k, 300, 8, 0.5, b.reg)
        if optimizer == "adagrad":
            ids, perm = ops.segment_sort_multi([u, i, j], [0, nu, nu], nu + ni)
            ops.sparse_adagrad_multi([b.user_factors, b.item_factors], [b.user_accum, b.item_accum], [0, nu, nu + ni], ids, perm,
                                     grads, b.lr)
        else:
            ids, perm = ops.segment_sort(u, nu)
            ops.sparse_sgd(b.user_factors, ids, perm, grads[:300], b.lr)
            ids, perm = ops.segment_sort(ops.concat_offset_ids([i, j], [0, 0]), ni)
            ops.sparse_sgd(b.item_factors, ids, perm, grads[300:], b.lr)
        n = int(valid.sum())
        want_loss.append(float(loss_t.to(torch.float64).sum()) / n if n else float("nan"))
        want_trials.append(float(trials.sum()) / 300)
    assert losses == want_loss and a.mean_trials == want_trials and a.step == 3 and np.isfinite(losses).all()
    for k in ("user_factors", "item_factors", "user_accum", "item_accum"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    u, i, j, valid, trials = a.step_triples()
    got = ops.warp_step(b.user_factors, b.item_factors, b._offsets_dev, b._row_upos, b._row_ipos, b.rank_weight, 5, 3, 300, 8, 0.5,
                        b.reg, want_grads=False)
    assert all(torch.equal(x, y) for x, y in zip((u, i, j, valid, trials), got[:5])) and a.step == 3
    assert torch.equal(a.user_factors, b.user_factors)                          # step_triples updates nothing


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_one_step_against_fp64(dev, optimizer):
    from esrecsys_amd.factorization import WARP
    user, item = _pairs(np.random.default_rng(42))
    m = WARP(user, item, rank=16, batch=512, seed=6, optimizer=optimizer, max_trials=16, margin=1.0, device=dev)
    U, Y = m.user_factors.cpu().numpy(), m.item_factors.cpu().numpy()
    Ua, Ya = m.user_accum.cpu().numpy(), m.item_accum.cpu().numpy()
    csr = (m._user_offsets, m._row_upos.cpu().numpy(), m._row_ipos.cpu().numpy())
    weight = m.rank_weight.cpu().numpy()
    assert np.array_equal(weight, wref.harmonic(m.items.numel()))
    args = (csr, weight, 6, 0, 512, 16, 1.0, m.reg, m.lr, optimizer)
    r64, r32 = wref.step_ref(U, Y, Ua, Ya, *args, np.float64), wref.step_ref(U, Y, Ua, Ya, *args, np.float32)
    assert not r64["undecided"].any() and wref.same_selection(r32, r64).all()   # a condition of this case
    u, i, j, valid, trials = (t.cpu().numpy() for t in m.step_triples())
    assert wref.same_selection(dict(zip(wref.IDS, (u, i, j, valid, trials))), r64).all()
    loss = m.train_steps(1)[0]
    keys = ("user", "item", "user_acc", "item_acc")
    bound, e32 = wref.bounds(r32, r64, keys)
    got = dict(zip(keys, (t.cpu().numpy() for t in (m.user_factors, m.item_factors, m.user_accum, m.item_accum))))
    for k in keys:
        err = wref.arr_err(got[k], r64[k])
        print("WARP step %s %s: error %.3g  e32 %.3g  bound %.3g" % (optimizer, k, err, e32[k], bound[k]))
        assert err <= bound[k], (k, err, e32[k], bound[k])
    e_loss = abs(r32["loss"] - r64["loss"]) / abs(r64["loss"])
    assert abs(loss - r64["loss"]) / abs(r64["loss"]) <= wref.FACTOR * e_loss + wref.FLOOR
    assert m.mean_trials == [r64["mean_trials"]]


def test_constructor_state_is_bprs_and_recommend_is_a_full_sort(dev):
    import torch
    from esrecsys_amd.factorization import BPR, WARP
    user, item = _pairs(np.random.default_rng(43))
    kw = dict(rank=8, reg=0.02, lr=0.1, batch=128, seed=9, device=dev)
    w, b = WARP(user, item, **kw), BPR(user, item, **kw)
    for k in ("users", "items", "user_factors", "item_factors", "user_accum", "item_accum", "_row_upos", "_row_ipos", "_key",
              "_offsets_dev"):
        assert torch.equal(getattr(w, k), getattr(b, k)), k
    for k in ("rank", "reg", "lr", "optimizer", "batch", "seed", "init_scale", "step", "nnz"):
        assert getattr(w, k) == getattr(b, k), k
    assert (w.max_trials, w.margin, w.mean_trials) == (32, 1.0, [])
    w.fit(5)
    assert w.step == 5 and len(w.mean_trials) == 5
    queries = w.users.cpu().numpy().astype(np.int64)[:20]
    items = w.items.cpu().numpy().astype(np.int64)
    full = w.score(np.repeat(queries, items.size), np.tile(items, queries.size)).cpu().numpy().reshape(queries.size, -1)
    ids, scores, lengths = (t.cpu().numpy() for t in w.recommend(queries, k=10, exclude_seen=False))
    for q in range(queries.size):
        order = np.lexsort((items, -full[q]))[:10]
        assert lengths[q] == 10 and np.array_equal(scores[q], full[q][order]) and np.array_equal(ids[q], items[order]), q


def test_learning_on_the_planted_corpus(dev):
    from esrecsys_amd.factorization import WARP
    from test_warp_ref import planted_start
    P = wref.PLANTED
    user, item = wref.planted_pairs()
    m = WARP(user, item, rank=P["rank"], batch=P["batch"], seed=P["seed"], reg=bref.REG, lr=bref.LR, device=dev,
             **wref.PLANTED_WARP)
    U0, Y0 = planted_start()
    assert np.array_equal(m.user_factors.cpu().numpy(), U0) and np.array_equal(m.item_factors.cpu().numpy(), Y0)
    _, want, _, _ = wref.planted_run(U0, Y0)
    before = m.auc()
    m.fit(P["steps"])
    after = m.auc()
    print("planted WARP: auc %.4f -> %.4f (fp64 reference %.4f), mean trials %.3f -> %.3f"
          % (before, after, want, m.mean_trials[0], m.mean_trials[-1]))
    assert after >= want - 0.02 and after > before
    assert m.mean_trials[-1] > m.mean_trials[0] and len(m.mean_trials) == P["steps"]

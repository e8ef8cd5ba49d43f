"""GPU: the triple family past one launch grid and at the constructor's default size.

Every kernel of the family walks its work with a grid-stride loop under a capped grid: past the cap a lane
group (or a sampler workgroup) takes a second item, `t` and the `B + t`, `2 B + t` gradient rows are large, and in the ragged
last pass some groups of a wave have left the loop while others still sum across their lanes.  The shapes here are the
smallest that cross each cap:

  bpr_fwd_bwd   2048 workgroups of 256 / G triples: B = 2048 (256 / G) + 257 at every lane-group width G = 1 .. 32, with the
                ranks whose last lanes hold nothing (12, 24, 36, 100) -- against calls over consecutive pieces bit for bit,
                and the second pass against fp64 under the rule of _bpr_ref (kernel error <= 4 e32 + 2^-22)
  BPR, HybridBPR at rank 64, batch 65 536 (the defaults: two passes of 32 768 triples in every step) against the ops
                composed by hand, and one BPR step against fp64 under the same rule
  warp_step     32 768 workgroups: B = 262 144 + 257 at G = 32 against the fp64 restatement bit for bit on exact tables
  the samplers  32 768 workgroups: K * ceil(B / 256) past it, against the restatements of chosen steps

Measured on an MI355X: profiles/triple_scale/ (README.md, parity_errors.json)."""
import json
import os

import numpy as np
import pytest

import _bpr_ref as bref
import _fpmc_ref as fref
import _sgns_ref as sref
import _warp_ref as wref
from conftest import rel_err
from test_gpu_bpr import _check_rule, _tables, _zipf_pairs

pytestmark = pytest.mark.gpu

MAX_GRID = 2048                 # kMaxGrid of esr_common.h: the workgroups of bpr_fwd_bwd
BLOCK = 256                     # kBlock
MAX_BLOCKS = 16 * MAX_GRID      # kSampledMaxBlocks (esr_sampled.h): warp_step and the three samplers
TAIL = 257
MEASURED = {}


def _t(dev, a, dt=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)


def _lanes(D):
    G = 1
    while G < D // 4:
        G *= 2
    return G


def _note(key, err, e32):
    """keep a measured error with its multiple of e32 and its share of the bound (the form of profiles/hybrid)"""
    MEASURED[key] = {"error": err, "e32": e32, "multiple_of_e32": err / e32 if e32 else 0.0,
                     "share_of_bound": err / (bref.FACTOR * e32 + bref.FLOOR)}
    path = os.environ.get("ESR_TRIPLE_SCALE_PARITY_JSON")   # (profiles/triple_scale/parity_errors.json: one run written this way)
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


# ---- 1. bpr_fwd_bwd past its grid, at every lane-group width -----------------------------------------------------------------
def _thirds(grads, B, rows):
    """the rows `rows` (a slice or an index tensor) of each third of grads [3 B, D]"""
    return [grads[part * B:(part + 1) * B][rows] for part in range(3)]


@pytest.mark.parametrize("D", [4, 8, 12, 16, 24, 36, 64, 100, 128])
def test_bpr_fwd_bwd_past_one_grid_equals_calls_over_pieces_and_fp64(dev, D):
    """G = 1, 2, 4, 4, 8, 16, 16, 32, 32.  One pass is 2048 (256 / G) triples; the 257 after it are the second pass, the
    last of them in a wave whose other groups have left the loop.  The pieces are 8193 triples at G <= 4 and 257 above, cut
    so that the last piece is the second pass alone."""
    import torch
    from esrecsys_amd import ops
    from esrecsys_amd.factorization import FAIL_BAD_POSITION
    G = _lanes(D)
    assert G == {4: 1, 8: 2, 12: 4, 16: 4, 24: 8, 36: 16, 64: 16, 100: 32, 128: 32}[D]
    one_pass = MAX_GRID * (BLOCK // G)
    B = one_pass + TAIL
    rng = np.random.default_rng([31, D])
    nu, ni, reg = 50, 60, 0.01
    U, Y = _tables(rng, nu, ni, D)
    u, i, j = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    valid = (rng.random(B) >= 0.05).astype(np.int32)
    valid[one_pass], valid[one_pass + 1] = 1, 0                               # the second pass starts with one of each
    bad_at = {"u": one_pass + 100, "i": one_pass + 163, "j": B - 1}           # where an id will lie outside its table
    valid[list(bad_at.values())] = 1
    Ud, Yd = _t(dev, U), _t(dev, Y)
    ud, id_, jd, vd = (_t(dev, a, np.int32) for a in (u, i, j, valid))
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    loss_t, d, grads = ops.bpr_fwd_bwd(Ud, Yd, ud, id_, jd, vd, reg, want_diff=True, failed=failed)
    assert tuple(grads.shape) == (3 * B, D)
    # split equality, bit for bit
    piece = 8193 if G <= 4 else TAIL
    cuts = list(range(0, one_pass, piece)) + [one_pass, B]
    parts = [ops.bpr_fwd_bwd(Ud, Yd, ud[a:b], id_[a:b], jd[a:b], vd[a:b], reg, want_diff=True, failed=failed)
             for a, b in zip(cuts[:-1], cuts[1:])]
    assert int(failed.item()) == 0 and cuts[-2] == one_pass and parts[-1][0].numel() == TAIL
    assert torch.equal(torch.cat([p[0] for p in parts]), loss_t) and torch.equal(torch.cat([p[1] for p in parts]), d)
    for part in range(3):
        pieces = torch.cat([p[2][part * p[0].numel():(part + 1) * p[0].numel()] for p in parts])
        assert torch.equal(pieces, grads[part * B:(part + 1) * B]), part
    # the second pass against fp64 under the rule
    tail = slice(B - TAIL, B)
    got = (loss_t[tail].cpu().numpy(), d[tail].cpu().numpy(), torch.cat(_thirds(grads, B, tail)).cpu().numpy())
    on = valid[tail] != 0
    assert on.any() and (~on).any()
    assert got[0][on].all() and not got[0][~on].any() and not got[1][~on].any() and not got[2][np.tile(~on, 3)].any()
    what = "past-grid-D%d-G%d-B%d" % (D, G, B)
    _check_rule(got, U, Y, u[tail], i[tail], j[tail], valid[tail], reg, what)
    r64 = bref.fwd_bwd_ref(U, Y, u[tail], i[tail], j[tail], valid[tail], reg, np.float64)
    r32 = bref.fwd_bwd_ref(U, Y, u[tail], i[tail], j[tail], valid[tail], reg, np.float32)
    for name, g, a, b in zip(("loss_t", "d", "grads"), got, r32, r64):
        _note("bpr_fwd_bwd/%s/%s" % (what, name), bref.arr_err(g, b), bref.arr_err(a, b))
    # one id outside its table in the second pass: bit 30, that triple's outputs zero, every other triple keeps its bits
    for name, ids, value in (("u", u, nu), ("i", i, -1), ("j", j, ni)):
        at = bad_at[name]
        assert bool(loss_t[at]) and all(bool(g[at].any()) for g in _thirds(grads, B, slice(None)))    # the clean call's
        bad = ids.copy()
        bad[at] = value
        args = {"u": ud, "i": id_, "j": jd}
        args[name] = _t(dev, bad, np.int32)
        failed.zero_()
        b_loss, b_d, b_grads = ops.bpr_fwd_bwd(Ud, Yd, args["u"], args["i"], args["j"], vd, reg, want_diff=True, failed=failed)
        assert int(failed.item()) == FAIL_BAD_POSITION == 1 << 30, name
        assert not bool(b_loss[at]) and not bool(b_d[at]) and not any(bool(g[at].any()) for g in _thirds(b_grads, B, slice(None)))
        others = torch.ones(B, dtype=torch.bool, device=dev)
        others[at] = False
        assert torch.equal(b_loss[others], loss_t[others]) and torch.equal(b_d[others], d[others]), name
        for got_third, want_third in zip(_thirds(b_grads, B, others), _thirds(grads, B, others)):
            assert torch.equal(got_third, want_third), name


# ---- 2. the default BPR and HybridBPR step -----------------------------------------------------------------------------------
DEFAULT = dict(nu=200, ni=300, rank=64, batch=65536)


def _default_bpr(dev, optimizer):
    from esrecsys_amd.factorization import BPR
    user, item = _zipf_pairs(np.random.default_rng(21), DEFAULT["nu"], DEFAULT["ni"], 12)
    m = BPR(user, item, optimizer=optimizer, seed=4, device=dev)              # rank and batch: the constructor's defaults
    assert (m.rank, m.batch) == (DEFAULT["rank"], DEFAULT["batch"]) and _lanes(m.rank) == 16
    assert m.batch == 2 * MAX_GRID * (BLOCK // 16)                            # two whole passes of bpr_fwd_bwd's grid
    return m


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_default_bpr_train_steps_equal_the_ops_composed_by_hand(dev, optimizer):
    import torch
    from esrecsys_amd import ops
    a, b = _default_bpr(dev, optimizer), _default_bpr(dev, optimizer)
    nu, ni, B = DEFAULT["nu"], DEFAULT["ni"], DEFAULT["batch"]
    assert torch.equal(a.user_factors, b.user_factors) and (a.users.numel(), a.items.numel()) == (nu, ni)
    losses = a.train_steps(2)
    u, i, j, valid, dropped = ops.bpr_sample(b._offsets_dev, b._row_upos, b._row_ipos, nu, ni, b.seed, 0, 2, B)
    by_hand = []
    for k in range(2):
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
    assert losses == by_hand and a.step == 2 and b.step == 0 and np.isfinite(losses).all()
    for x, y in ((a.user_factors, b.user_factors), (a.item_factors, b.item_factors), (a.user_accum, b.user_accum),
                 (a.item_accum, b.item_accum)):
        assert torch.equal(x, y)
    assert all(torch.equal(x, y) for x, y in zip(a.sample(1), a.sample(1, step0=2)))


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_default_bpr_one_step_against_fp64(dev, optimizer):
    m = _default_bpr(dev, optimizer)
    nu, ni, B = DEFAULT["nu"], DEFAULT["ni"], DEFAULT["batch"]
    start = {k: getattr(m, a).cpu().numpy() for k, a in (("user", "user_factors"), ("item", "item_factors"),
                                                         ("user_acc", "user_accum"), ("item_acc", "item_accum"))}
    u, i, j, valid, dropped = (t.cpu().numpy() for t in m.sample(1))
    second = slice(B // 2, B)                                                 # the second pass of the launch
    assert valid[0][second].any() and dropped[0] == (valid[0] == 0).sum() and (m.users.numel(), m.items.numel()) == (nu, ni)
    assert len(np.unique(i[0])) <= ni < B // 4                                # ids repeat: long runs for the update
    loss = m.train_steps(1)[0]
    ref = {dtype: bref.step_ref(start["user"], start["item"], start["user_acc"], start["item_acc"], u[0], i[0], j[0], valid[0],
                                m.reg, m.lr, optimizer, dtype) for dtype in (np.float64, np.float32)}
    keys = ("user", "item") + (("user_acc", "item_acc") if optimizer == "adagrad" else ())
    bound, e32 = bref.bounds(ref[np.float32], ref[np.float64], keys)
    got = {"user": m.user_factors, "item": m.item_factors, "user_acc": m.user_accum, "item_acc": m.item_accum}
    for key in keys:
        err = rel_err(got[key].cpu().numpy(), ref[np.float64][key])
        print("default bpr step %s %s: error %.3g  e32 %.3g  bound %.3g" % (optimizer, key, err, e32[key], bound[key]))
        _note("bpr_step/default-%s/%s" % (optimizer, key), err, e32[key])
        assert err <= bound[key], (key, err, e32[key], bound[key])
    want = ref[np.float64]["loss"]
    e = abs(ref[np.float32]["loss"] - want) / want
    err = abs(loss - want) / want
    print("default bpr step %s loss: error %.3g  e32 %.3g" % (optimizer, err, e))
    _note("bpr_step/default-%s/loss" % optimizer, err, e)
    assert err <= bref.FACTOR * e + bref.FLOOR, (err, e)
    if optimizer == "sgd":
        assert np.array_equal(m.user_accum.cpu().numpy(), start["user_acc"])


@pytest.mark.parametrize("optimizer", ["adagrad", "sgd"])
def test_default_hybrid_train_step_equals_the_ops_composed_by_hand(dev, optimizer):
    """HybridBPR at its defaults: bpr_fwd_bwd unchanged over the composed rows P [B, 64] and Q [2 B, 64], two passes"""
    import torch
    from esrecsys_amd import ops
    from esrecsys_amd.factorization import HybridBPR
    nu, ni = DEFAULT["nu"], DEFAULT["ni"]
    user, item = _zipf_pairs(np.random.default_rng(21), nu, ni, 12)
    rng = np.random.default_rng(22)
    # a category for every item, a tag with a weight for every third one; a group for every other user
    tagged = np.arange(0, ni, 3)
    ent = np.concatenate([np.arange(ni), tagged])
    fid = np.concatenate([1000 + np.arange(ni) % 9, 2000 + rng.integers(0, 30, tagged.size)])
    weight = (2.0 ** rng.integers(-2, 2, ent.size)).astype(np.float32)
    grouped = np.arange(0, nu, 2)

    def model():
        return HybridBPR(user, item, user_features=(grouped, 50 + grouped % 5, None), item_features=(ent, fid, weight),
                         optimizer=optimizer, seed=4, device=dev)
    a, b = model(), model()
    B = b.batch
    assert (b.rank, B) == (DEFAULT["rank"], DEFAULT["batch"]) and (b.users.numel(), b.items.numel()) == (nu, ni)
    nfu, nfi = b.user_embeddings.shape[0], b.item_embeddings.shape[0]
    assert nfu == nu + 5 and nfi > ni + 9
    losses = a.train_steps(1)
    u, i, j, valid, dropped = b.sample(1)
    ar = torch.arange(2 * B, dtype=torch.int32, device=dev)
    ij, v2 = torch.cat([i[0], j[0]]), torch.cat([valid[0], valid[0]])
    P = ops.bag_sum(b.user_embeddings, *b._user_bags.args(), rows=u[0])
    Q = ops.bag_sum(b.item_embeddings, *b._item_bags.args(), rows=ij)
    loss_t, _, grads = ops.bpr_fwd_bwd(P, Q, ar[:B], ar[:B], ar[B:], valid[0], 0.0)
    oo_u = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(b._user_bags.lengths[u[0].long()], 0)])
    oo_i = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(b._item_bags.lengths[ij.long()], 0)])
    fu, gu = ops.bag_expand(b.user_embeddings, *b._user_bags.args(), u[0], grads[:B], valid[0], oo_u, int(oo_u[-1]), b.reg)
    fi, gi = ops.bag_expand(b.item_embeddings, *b._item_bags.args(), ij, grads[B:], v2, oo_i, int(oo_i[-1]), b.reg)
    if optimizer == "adagrad":
        s, p = ops.segment_sort_multi([fu, fi], [0, nfu], nfu + nfi)
        ops.sparse_adagrad_multi([b.user_embeddings, b.item_embeddings], [b.user_accum, b.item_accum], [0, nfu, nfu + nfi],
                                 s, p, torch.cat([gu, gi]), b.lr)
    else:
        s, p = ops.segment_sort(fu, nfu)
        ops.sparse_sgd(b.user_embeddings, s, p, gu, b.lr)
        s, p = ops.segment_sort(fi, nfi)
        ops.sparse_sgd(b.item_embeddings, s, p, gi, b.lr)
    by_hand = [float(loss_t.to(torch.float64).sum()) / (B - int(dropped[0]))]
    assert losses == by_hand and np.isfinite(losses).all() and a.step == 1 and b.step == 0
    assert bool(loss_t[B // 2:].any()) and int(dropped[0]) < B
    for x, y in ((a.user_embeddings, b.user_embeddings), (a.item_embeddings, b.item_embeddings), (a.user_accum, b.user_accum),
                 (a.item_accum, b.item_accum)):
        assert torch.equal(x, y)
    assert not torch.equal(a.item_embeddings, model().item_embeddings)


# ---- 3. warp_step past kSampledMaxBlocks ----------------------------------------------------------------------------------------
WARP_ONE_PASS = MAX_BLOCKS * (BLOCK // 32)          # 262 144 slots: 32 768 workgroups of 8 groups of 32 lanes
WARP_T = 5
_WARP = {}


def _warp_case(D):
    """the T = 5 case of _warp_ref.exact_grid_cases(D) (exact tables and weights, nu = 23, ni = 97, CSR rows of 1, 3, 17 and
    40 items, margin = the multiple of 2^-6 next to the 2 / T quantile of d, reg = 2^-6) at B = 262 144 + 257, and its fp64
    restatement on the first 257 slots, the 514 around the cap and the last 257 -- computed once"""
    if D not in _WARP:
        B = WARP_ONE_PASS + TAIL
        case = dict(next(c for c in wref.exact_grid_cases(D) if c["T"] == WARP_T), B=B, name="past-grid-D%d" % D)
        groups = {"first": np.arange(TAIL), "cap": np.arange(WARP_ONE_PASS - TAIL, WARP_ONE_PASS + TAIL),
                  "last": np.arange(B - TAIL, B)}
        refs = {k: wref.warp_ref(case["user"], case["item"], case["csr"], case["weight"], case["seed"], case["step"], B,
                                 case["T"], case["margin"], case["reg"], np.float64, slots=s) for k, s in groups.items()}
        _WARP[D] = (case, groups, refs)
    return _WARP[D]


def _warp_first_candidate_seen(case, slots, r):
    """bool per slot: the first candidate of the stream (always walked) is an item the user has seen"""
    off, _, ipos = (np.asarray(a, np.int64) for a in case["csr"])
    ni = case["item"].shape[0]
    words = wref.stream_words(case["seed"], case["step"], case["B"], case["T"] + 1, slots=slots)
    cand = ((words[:, 1] * np.uint64(ni)) >> np.uint64(32)).astype(np.int64)
    u = r["u"].astype(np.int64)
    return bref._row_has(ipos, off[u], off[u + 1], cand)


def _warp_run(dev, case, B):
    import torch
    from esrecsys_amd import ops
    off, upos, ipos = case["csr"]
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = ops.warp_step(_t(dev, case["user"]), _t(dev, case["item"]), _t(dev, off, np.int64), _t(dev, upos, np.int32),
                        _t(dev, ipos, np.int32), _t(dev, case["weight"], np.float32), case["seed"], case["step"], B, case["T"],
                        float(case["margin"]), float(case["reg"]), want_diff=True, failed=failed)
    return dict(zip(wref.IDS + wref.ARRAYS, out)), int(failed.item())


@pytest.mark.parametrize("D", [128, 100])
def test_warp_step_past_its_block_cap_bit_for_bit(dev, D):
    """G = 32: 8 slots per workgroup and at most 32 768 workgroups, so slot 262 144 is the first of a second pass.  The
    narrower widths share the loop (`for (t = row4_first<G>(); t < B; t += ngroups)`) but reach the cap only at 0.5 M
    (G = 16) to 8.4 M slots (G = 1), more than a test can afford: they are not run here.  The 400 MB of gradient rows stay
    on the device; the reference slots are sliced there."""
    import torch
    case, groups, refs = _warp_case(D)
    B = case["B"]
    assert _lanes(D) == 32 and B == WARP_ONE_PASS + TAIL and case["user"].shape == (23, D) and case["item"].shape == (97, D)
    # conditions on the reference, checked on the CPU first
    last = refs["last"]
    assert set(last["valid"].tolist()) == {0, 1} and (last["trials"] == 1).any() and (last["trials"] > 1).any()
    seen_first = _warp_first_candidate_seen(case, groups["last"], last)
    assert seen_first.any() and not last["bad"]                               # a candidate skipped as seen
    got, word = _warp_run(dev, case, B)
    assert word == 0 and tuple(got["grads"].shape) == (3 * B, D)
    for name, slots in groups.items():
        at = _t(dev, slots)
        r = refs[name]
        for k in wref.IDS:
            g = got[k][at].cpu().numpy()
            assert g.dtype == np.int32 and np.array_equal(g, r[k]), (name, k)
        for k in ("loss_t", "d"):
            g = got[k][at].cpu().numpy()
            assert g.dtype == np.float32 and np.array_equal(g, r[k].astype(np.float32)), (name, k)
        g = torch.cat(_thirds(got["grads"], B, at)).cpu().numpy()
        assert g.dtype == np.float32 and np.array_equal(g, r["grads"].astype(np.float32)), (name, "grads")
    assert bool(got["loss_t"][WARP_ONE_PASS:].any()) and bool(got["grads"][3 * B - TAIL:].any())
    # independence of the launch: exactly one pass equals the first 262 144 slots of the two-pass call
    one, word = _warp_run(dev, case, WARP_ONE_PASS)
    assert word == 0
    for k in wref.IDS + ("loss_t", "d"):
        assert torch.equal(one[k], got[k][:WARP_ONE_PASS]), k
    for part, (a, b) in enumerate(zip(_thirds(one["grads"], WARP_ONE_PASS, slice(None)),
                                      _thirds(got["grads"], B, slice(0, WARP_ONE_PASS)))):
        assert torch.equal(a, b), part


# ---- 4. the three samplers past their block cap ----------------------------------------------------------------------------
# (B, K, step0): one workgroup per step and five steps in the second round (the step wraps 2^32 there); two workgroups per
# step, the second with one live thread, so that the cap falls on a step boundary
SAMPLER_SHAPES = [(1, MAX_BLOCKS + 5, 2 ** 32 - MAX_BLOCKS - 2), (257, MAX_BLOCKS // 2 + 3, 17)]


def _checked_steps(B, K):
    """[(k0, n)]: the first 3 steps, the 6 around the cap and the last 3"""
    per_step = -(-B // BLOCK)
    assert K * per_step > MAX_BLOCKS and MAX_BLOCKS % per_step == 0
    cap = MAX_BLOCKS // per_step                                              # the first step of the second round
    assert cap + 3 <= K
    return [(0, 3), (cap - 3, 6), (K - 3, 3)]


def _sampler_past_the_cap(dev, B, K, step0, names, sample, restate):
    """sample(step0, K, B) -> device tensors (..., dropped); restate(step0, K, B) -> the same arrays from the reference"""
    import torch
    got = sample(step0, K, B)
    valid, dropped = got[names.index("valid")], got[-1]
    assert tuple(dropped.shape) == (K,) and torch.equal(dropped, (valid == 0).sum(1).to(torch.int32))
    for k0, n in _checked_steps(B, K):
        want = restate((step0 + k0) % 2 ** 32, n, B)
        for name, g, w in zip(names, got, want):
            g = g[k0:k0 + n].cpu().numpy()
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (name, k0)
    return got


@pytest.mark.parametrize("B,K,step0", SAMPLER_SHAPES)
def test_bpr_sampler_past_its_block_cap(dev, B, K, step0):
    from esrecsys_amd import ops
    from test_gpu_bpr import ROW_LENGTHS
    nu, ni, seed = 9, 1001, (0xC0FFEE << 32) | 99
    csr = bref.random_csr(np.random.default_rng(11), nu, ni, ROW_LENGTHS)      # boundary_csr of test_gpu_bpr.py
    csr_d = tuple(_t(dev, a) for a in csr)
    _sampler_past_the_cap(dev, B, K, step0, "u i j valid dropped".split(),
                          lambda s, k, b: ops.bpr_sample(*csr_d, nu, ni, seed, s, k, b),
                          lambda s, k, b: bref.sample_ref(*csr, nu, ni, seed, s, k, b))


@pytest.mark.parametrize("B,K,step0", SAMPLER_SHAPES)
def test_fpmc_sampler_past_its_block_cap(dev, B, K, step0):
    from esrecsys_amd import ops
    from test_gpu_fpmc import ROW_LENGTHS, SEQ_LENGTHS
    rng = np.random.default_rng(11)                                           # boundary_csrs of test_gpu_fpmc.py
    (so, su, si), _ = fref.seq_csr({u: rng.integers(0, 1001, n).tolist() for u, n in enumerate(SEQ_LENGTHS)}, 7)
    ro, _, ri = bref.random_csr(rng, 7, 1001, ROW_LENGTHS)
    csrs = (so, su, si, ro, ri)
    csrs_d = tuple(_t(dev, a) for a in csrs)
    nu, ni, window, seed = 7, 1001, 3, (0xC0FFEE << 32) | 99
    got = _sampler_past_the_cap(dev, B, K, step0, "u e c i j valid dropped".split(),
                                lambda s, k, b: ops.fpmc_sample(*csrs_d, nu, ni, window, seed, s, k, b),
                                lambda s, k, b: fref.sample_ref(*csrs, nu, ni, window, seed, s, k, b))
    assert int(got[2].max()) <= window


@pytest.mark.parametrize("B,K,step0", SAMPLER_SHAPES)
def test_sgns_sampler_past_its_block_cap(dev, B, K, step0):
    from esrecsys_amd import ops
    (so, su, si), nd, ni, keep, alias = sref.boundary_corpus()                # corpus of test_gpu_sgns.py
    window, negatives, seed = 5, 5, (0xC0FFEE << 32) | 99
    dev_args = (_t(dev, so), _t(dev, su), _t(dev, si), nd, ni, window, negatives, _t(dev, keep.view(np.int32)), _t(dev, alias))

    def sample(s, k, b):
        c, e, o, valid, neg, dropped = ops.sgns_sample(*dev_args, seed, s, k, b)
        assert tuple(neg.shape) == (k, b, negatives)
        return c, e, o, valid, neg, dropped

    def restate(s, k, b):
        return sref.sample_ref(so, su, si, nd, ni, window, negatives, keep, alias, seed, s, k, b)
    got = _sampler_past_the_cap(dev, B, K, step0, "c e o valid neg dropped".split(), sample, restate)
    assert int(got[4].min()) >= 0 and int(got[4].max()) < ni

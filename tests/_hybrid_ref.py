"""Plain NumPy restatement of the bag rules of esr_bag_rule.h and of one whole step of factorization.HybridBPR.  No GPU, no
torch: tests/test_hybrid_ref.py checks it on the CPU, tests/test_gpu_hybrid.py runs the kernels against it.

Two flavours, chosen by `dtype`:
    np.float64   every product and sum in fp64;
    np.float32   the chain the kernels run, restated as  acc = float32(float64(w) * float64(e) + float64(acc))  per step.
A product of two float32 is exact in fp64.  On EXACT cases -- tables whose entries are multiples of 2^-6 below 2^6 in
magnitude (``exact_table``), weights that are signed powers of two in [2^-3, 2^3] (``exact_weights``), and the order
witnesses +-2^25 and 1 -- every partial sum is a multiple of 2^-9 below 2^40 and exact in fp64 too, so the restated step
rounds once, as fmaf does: the float32 flavour then equals the kernels bit for bit.  On random tables the fp64 sum may round
before the float32 rounding does (a double rounding, rare); there the rule of tests/_bpr_ref.py holds:

    kernel error against fp64  <=  FACTOR * e32 + 2^-22,   e32 = error of the float32 flavour against fp64

(arrays: max |a - b| / max |b|: the row's scale is the largest entry of the array).  FACTOR = 4 as for BPR and WARP; the
kernels run the very chain the float32 flavour restates, so the measured multiple is about 1
(profiles/hybrid/parity_errors.json).
"""
import numpy as np

import _bpr_ref as bref
from oracle import optim as o_optim

FACTOR, FLOOR = bref.FACTOR, bref.FLOOR
LENGTHS = (1031, 0, 1, 2, 63, 64, 65, 257)      # bag b of a grid table has LENGTHS[b % 8] occurrences
WITNESS = (1.0, 2.0 ** 25, -2.0 ** 25)          # in this order the chain gives 0, reversed it gives 1


def _span(offsets, b, nnz):
    lo = np.clip(offsets[b], 0, nnz)
    hi = np.clip(offsets[b + 1], lo, nnz)
    return lo, hi


def _selected(offsets, rows, n_bags):
    """(bag numbers int64[n], ok bool[n]) of `rows` (None: every bag in order)"""
    b = np.arange(n_bags, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    return b, (b >= 0) & (b < n_bags)


def _fma(w, e, acc, dtype):
    """one chain step on arrays: fp64 throughout, or rounded to float32 once per step"""
    v = w.astype(np.float64) * e.astype(np.float64) + acc.astype(np.float64)
    return v.astype(dtype)


def bag_sum_ref(table, offsets, feat, weight, rows, dtype):
    """(out [n, D] in `dtype`, failed bool): esr_bag_sum by the rule.  A bag number outside [0, n_bags) or a feature
    position outside [0, nf) gives a zero row and failed."""
    table = np.asarray(table).astype(dtype)                             # (float32 tables pass through unchanged)
    offsets, feat = np.asarray(offsets, np.int64), np.asarray(feat, np.int64)
    nf, D, nnz, n_bags = table.shape[0], table.shape[1], feat.size, offsets.size - 1
    b, ok = _selected(offsets, rows, n_bags)
    safe = np.where(ok, b, 0)
    lo, hi = _span(offsets, safe, nnz)
    hi = np.where(ok, hi, lo)
    w_all = np.ones(nnz, np.float32) if weight is None else np.asarray(weight, np.float32)
    good = (feat >= 0) & (feat < nf)
    acc = np.zeros((b.size, D), dtype)
    bad = ~ok
    for t in range(int((hi - lo).max()) if b.size else 0):
        live = np.flatnonzero(lo + t < hi)
        k = lo[live] + t
        bad[live] |= ~good[k]
        e = table[np.where(good[k], feat[k], 0)]
        acc[live] = _fma(w_all[k][:, None], e, acc[live], dtype)
    acc[bad] = 0
    return acc, bool(bad.any())


def out_offsets_ref(offsets, rows, nnz=None):
    """int64[n + 1]: the exclusive scan of the selected bags' lengths (a bag number outside the table counts 0)"""
    offsets = np.asarray(offsets, np.int64)
    n_bags = offsets.size - 1
    nnz = int(offsets[-1]) if nnz is None else nnz
    b, ok = _selected(offsets, rows, n_bags)
    lo, hi = _span(offsets, np.where(ok, b, 0), nnz)
    return np.concatenate([[0], np.cumsum(np.where(ok, hi - lo, 0))]).astype(np.int64)


def bag_expand_ref(table, offsets, feat, weight, rows, grad_rows, valid, reg, dtype):
    """(out_feat int32[M], out_grads [M, D] in `dtype`, out_offsets int64[n + 1], failed bool): esr_bag_expand by the
    rule, with out_offsets computed as the caller does."""
    table, grad_rows = np.asarray(table).astype(dtype), np.asarray(grad_rows).astype(dtype)
    offsets, feat = np.asarray(offsets, np.int64), np.asarray(feat, np.int64)
    nf, D, nnz, n_bags = table.shape[0], table.shape[1], feat.size, offsets.size - 1
    b, ok = _selected(offsets, rows, n_bags)
    oo = out_offsets_ref(offsets, rows, nnz)
    M = int(oo[-1])
    lo, _ = _span(offsets, np.where(ok, b, 0), nnz)
    r = np.repeat(np.arange(b.size), np.diff(oo))                       # the selected bag of every output row
    k = lo[r] + (np.arange(M) - oo[r])
    good = (feat[k] >= 0) & (feat[k] < nf)
    live = np.ones(b.size, bool) if valid is None else np.asarray(valid) != 0
    w = np.ones(M, np.float32) if weight is None else np.asarray(weight, np.float32)[k]
    e = table[np.where(good, feat[k], 0)]
    if dtype == np.float64:
        rows_out = w[:, None].astype(np.float64) * grad_rows[r] + np.float64(np.float32(reg)) * e
    else:
        l2 = (np.float64(np.float32(reg)) * e.astype(np.float64)).astype(np.float32)         # reg * e, rounded once
        rows_out = _fma(w[:, None], grad_rows[r], l2, np.float32)
    keep = good & live[r]
    rows_out = np.where(keep[:, None], rows_out, 0).astype(dtype)
    out_feat = np.where(good, feat[k], 0).astype(np.int32)
    return out_feat, rows_out, oo, bool((~good).any() or (~ok).any())


# ---- exact cases -----------------------------------------------------------------------------------------------------------
def exact_table(rng, nf, D):
    """float32 [nf + 3, D]: multiples of 2^-6 below 2^6 in magnitude; the last three rows are the order witnesses
    (all ones, all 2^25, all -2^25)."""
    body = rng.integers(-4095, 4096, (nf, D)).astype(np.float32) / np.float32(64.0)
    return np.concatenate([body, np.repeat(np.array(WITNESS, np.float32)[:, None], D, 1)])


def exact_weights(rng, n):
    """signed powers of two in [2^-3, 2^3]"""
    return (np.float32(2.0) ** rng.integers(-3, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def grid_bags(rng, n_bags, nf, lengths=LENGTHS):
    """(offsets, feat, weight): bag b has lengths[b % len] occurrences of random features of [0, nf); every bag of three or
    more occurrences holds the witness rows nf, nf + 1, nf + 2 (weight 1) at consecutive places, the start moving with b so
    that the triple meets every residue of any unroll."""
    lens = np.array([lengths[b % len(lengths)] for b in range(n_bags)], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feat = rng.integers(0, nf, int(offsets[-1])).astype(np.int32)
    weight = exact_weights(rng, feat.size)
    for b in np.flatnonzero(lens >= 3):
        at = offsets[b] + (b // len(lengths) + b) % (lens[b] - 2)
        feat[at:at + 3] = [nf, nf + 1, nf + 2]
        weight[at:at + 3] = 1.0
    return offsets, feat, weight


# ---- one whole step --------------------------------------------------------------------------------------------------------
def step_ref(ue, ie, ua, ia, ubag, ibag, u, i, j, valid, reg, lr, optimizer, dtype, eps=bref.EPS):
    """One step of HybridBPR in `dtype`: compose, BPR's forward / backward on the composed rows with reg = 0, expand with
    the model's reg, row-sparse Adagrad (oracle.optim) or SGD per table.  ubag / ibag = (offsets, feat, weight or None).
    A dict with loss_t, loss, the per-occurrence (feat, grads) of each side and the tables and accumulators after."""
    B = len(u)
    ij = np.concatenate([np.asarray(i, np.int64), np.asarray(j, np.int64)])
    P, _ = bag_sum_ref(ue, *ubag, u, dtype)
    Q, _ = bag_sum_ref(ie, *ibag, ij, dtype)
    ar = np.arange(B)
    loss_t, d, grads = bref.fwd_bwd_ref(P, Q, ar, ar, B + ar, valid, 0.0, dtype)
    valid2 = None if valid is None else np.concatenate([valid, valid])
    # (the expansion reads float32 gradient rows on the device; the fp64 flavour keeps them in fp64)
    fu, gu = _expand_any(ue, ubag, u, grads[:B], valid, reg, dtype)
    fi, gi = _expand_any(ie, ibag, ij, grads[B:], valid2, reg, dtype)
    E = {"user": np.asarray(ue).astype(dtype), "item": np.asarray(ie).astype(dtype)}
    A = {"user": np.asarray(ua).astype(dtype), "item": np.asarray(ia).astype(dtype)}
    for side, f, g in (("user", fu, gu), ("item", fi, gi)):
        if optimizer == "adagrad":
            E[side], A[side] = o_optim.sparse_adagrad_update(E[side], A[side], f, g, lr, eps, dtype=dtype)
        else:
            uniq, summed = o_optim.segment_sum_rows(f, g, dtype)
            E[side][uniq] = E[side][uniq] - dtype(lr) * summed
    n_valid = B if valid is None else int((np.asarray(valid) != 0).sum())
    loss = float(np.sum(loss_t, dtype=np.float64)) / n_valid if n_valid else float("nan")
    return {"loss_t": loss_t, "d": d, "loss": loss, "user_feat": fu, "user_grads": gu, "item_feat": fi, "item_grads": gi,
            "user": E["user"], "item": E["item"], "user_acc": A["user"], "item_acc": A["item"]}


def _expand_any(table, bag, rows, grad_rows, valid, reg, dtype):
    """bag_expand_ref on gradient rows of `dtype` (the fp64 flavour must not round them to float32 first)"""
    offsets, feat, weight = bag
    table = np.asarray(table)
    offsets, feat = np.asarray(offsets, np.int64), np.asarray(feat, np.int64)
    oo = out_offsets_ref(offsets, rows, feat.size)
    rows = np.asarray(rows, np.int64)
    r = np.repeat(np.arange(rows.size), np.diff(oo))
    k = offsets[rows][r] + (np.arange(int(oo[-1])) - oo[r])
    w = np.ones(k.size, dtype) if weight is None else np.asarray(weight)[k].astype(dtype)
    live = np.ones(rows.size, bool) if valid is None else np.asarray(valid) != 0
    e = table[feat[k]].astype(dtype)
    if dtype == np.float64:
        out = w[:, None] * grad_rows[r] + np.float64(np.float32(reg)) * e
    else:
        out = _fma(w[:, None], grad_rows[r], (np.float32(reg) * e).astype(np.float32), np.float32)
    return feat[k].astype(np.int64), np.where(live[r][:, None], out, 0).astype(dtype)


def dense_gradient(nf, feat, grads):
    """the per-occurrence rows segment-summed per feature: float64 [nf, D]"""
    out = np.zeros((nf, grads.shape[1]), np.float64)
    np.add.at(out, np.asarray(feat, np.int64), np.asarray(grads, np.float64))
    return out


def identity_bags(n):
    return np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), None


# ---- the planted corpus of the learning tests ---------------------------------------------------------------------------
PLANTED = dict(clusters=4, users_per=16, items_per=20, withheld_per=2, seen=14, rank=8, batch=256, steps=150, seed=5, k=6,
               lr=0.05, reg=0.01)


def planted():
    """64 users and 80 items in 4 clusters; a user has seen 14 of the 18 training items of its cluster; 2 items per cluster
    (a tenth) are withheld from the pairs.  Every item carries its cluster's feature 100 + c.  Returns a dict: user, item
    (the pairs), feat_item / feat_id (features of the training items), new_item / new_feat (the withheld ones), cluster_of
    (per item id) and user_cluster."""
    P = PLANTED
    rng = np.random.default_rng(0)
    C, up, ip, wp = P["clusters"], P["users_per"], P["items_per"], P["withheld_per"]
    cluster_of = np.repeat(np.arange(C), ip)
    withheld = np.concatenate([c * ip + np.arange(ip - wp, ip) for c in range(C)])
    train = np.setdiff1d(np.arange(C * ip), withheld)
    user, item = [], []
    for u in range(C * up):
        c = u // up
        own = train[cluster_of[train] == c]
        seen = rng.choice(own, P["seen"], replace=False)
        user += [u] * P["seen"]
        item += seen.tolist()
    user, item = np.array(user, np.int64), np.array(item, np.int64)
    assert np.array_equal(np.unique(item), train)                      # every training item is seen by somebody
    return dict(user=user, item=item, feat_item=train, feat_id=100 + cluster_of[train], new_item=withheld,
                new_feat=100 + cluster_of[withheld], cluster_of=cluster_of, user_cluster=np.arange(C * up) // up)


def planted_chance():
    """the expected share of a user's own withheld items in a random top k of its unseen candidates"""
    P = PLANTED
    candidates = P["clusters"] * P["items_per"] - P["seen"]
    return P["k"] / candidates


def own_withheld_recall(rec_ids, corpus):
    """mean over users of the share of the user's cluster's withheld items among its k recommendations"""
    hits = []
    for u, row in enumerate(np.asarray(rec_ids)):
        own = corpus["new_item"][corpus["cluster_of"][corpus["new_item"]] == corpus["user_cluster"][u]]
        hits.append(np.isin(own, row).mean())
    return float(np.mean(hits))


def planted_reference_recall():
    """The fp64 restatement trained on the planted corpus for PLANTED['steps'] steps (sample_ref + step_ref, Adagrad), then
    every user's top k of its unseen training items and the composed withheld items: the recall own_withheld_recall
    measures."""
    P, c = PLANTED, planted()
    nu = P["clusters"] * P["users_per"]
    items = np.unique(c["item"])
    ni = items.size
    ipos = np.searchsorted(items, c["item"])
    off, upos, rpos = bref.csr_of({u: ipos[c["user"] == u].tolist() for u in range(nu)}, nu)
    fids = np.unique(c["feat_id"])
    # item bags: identity row first, then the cluster feature (rows ni ..)
    feat = np.stack([np.arange(ni), ni + np.searchsorted(fids, c["feat_id"])], 1).reshape(-1).astype(np.int32)
    ibag = (np.arange(0, 2 * ni + 1, 2, dtype=np.int64), feat, None)
    ubag = identity_bags(nu)
    rng = np.random.default_rng(1)
    s = P["rank"] ** -0.5
    ue, ie = rng.standard_normal((nu, P["rank"])) * s, rng.standard_normal((ni + fids.size, P["rank"])) * s
    ua, ia = np.full_like(ue, bref.ACC0), np.full_like(ie, bref.ACC0)
    u, i, j, valid, _ = bref.sample_ref(off, upos, rpos, nu, ni, P["seed"], 0, P["steps"], P["batch"])
    for k in range(P["steps"]):
        r = step_ref(ue, ie, ua, ia, ubag, ibag, u[k], i[k], j[k], valid[k], P["reg"], P["lr"], "adagrad", np.float64)
        ue, ie, ua, ia = r["user"], r["item"], r["user_acc"], r["item_acc"]
    X = ue
    Y = ie[:ni] + ie[ni + np.searchsorted(fids, c["feat_id"])]
    Ynew = ie[ni + np.searchsorted(fids, c["new_feat"])]
    scores = X @ np.concatenate([Y, Ynew]).T
    scores[c["user"], ipos] = -np.inf
    ids = np.concatenate([items, c["new_item"]])
    top = np.argsort(-scores, axis=1, kind="stable")[:, :P["k"]]
    return own_withheld_recall(ids[top], c)

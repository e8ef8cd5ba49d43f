"""Plain NumPy reference of the Factorised Personalised Markov Chain as esr_fpmc.hip and factorization.FPMC compute it: the
slot sampler of esr_fpmc_sample.h restated line by line, one step (per-slot loss, score difference, the 5 + c gradient rows,
row-sparse Adagrad or SGD on the four tables through oracle.optim), the planted chain of the learning tests and the
tolerance rule.  No GPU, no torch: tests/test_fpmc_ref.py checks all of it on the CPU, tests/test_gpu_fpmc.py runs the
kernels against it.

The tolerance rule is _bpr_ref's, for its reasons (the kernel's dot product is eight fmaf per lane and a butterfly, NumPy
sums pairwise; the context vector is a chain of c <= 8 fmaf against NumPy's multiply and add):

    kernel error against fp64  <=  4 * e32 + 2^-22,   e32 = error of the SAME restatement run in float32 against fp64
"""
import numpy as np

import _bpr_ref as bref
from _spotify_sampler_ref import philox4x32_10
from oracle import optim as o_optim

MAX_WINDOW = 8
MAX_TRIES = bref.MAX_TRIES
FLOOR, FACTOR = bref.FLOOR, bref.FACTOR
LR, EPS, REG, ACC0 = bref.LR, bref.EPS, bref.REG, bref.ACC0
TABLES = ("user", "item", "next", "prev")
arr_err = bref.arr_err


def bounds(r32, r64, keys):
    """{quantity: 4 * e32 + 2^-22} and the e32 themselves: the rule of _bpr_ref.bounds"""
    return bref.bounds(r32, r64, keys)


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def seq_csr(seqs, nu):
    """(seq_offsets int64[nu + 1], seq_upos, seq_ipos int32) of {user position: the items in time order}, and the seen CSR
    (row_offsets, row_ipos) of the same events"""
    upos, ipos, off = [], [], [0]
    for u in range(nu):
        items = list(seqs.get(u, ()))
        upos += [u] * len(items)
        ipos += items
        off.append(len(upos))
    row_offsets, _, row_ipos = bref.csr_of(seqs, nu)
    return (np.array(off, np.int64), np.array(upos, np.int32), np.array(ipos, np.int32)), (row_offsets, row_ipos)


def sample_ref(seq_offsets, seq_upos, seq_ipos, row_offsets, row_ipos, nu, ni, window, seed, step0, K, B):
    """(u, e, c, i, j, valid) int32 [K, B] and dropped int32[K] by the rule of esr_fpmc_sample.h."""
    seq_offsets, seq_upos, seq_ipos, row_offsets, row_ipos = (np.asarray(a, np.int64) for a in
                                                              (seq_offsets, seq_upos, seq_ipos, row_offsets, row_ipos))
    nnz_seq, nnz_seen = seq_upos.size, row_ipos.size
    assert 1 <= nnz_seq <= 2 ** 31 - 1 and 1 <= ni <= 2 ** 31 - 1 and seq_offsets.size == nu + 1 == row_offsets.size
    assert 1 <= window <= MAX_WINDOW
    seed = int(seed) & (2 ** 64 - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    out = np.zeros((6, K, B), np.int32)
    t = np.arange(B, dtype=np.uint64)
    for k in range(K):
        s = (int(step0) + k) & 0xFFFFFFFF
        counter = np.zeros((B, 4, 4), np.uint64)          # [slot, block, counter word] = (t, s, b, 0)
        counter[:, :, 0] = t[:, None]
        counter[:, :, 1] = s
        counter[:, :, 2] = np.arange(4, dtype=np.uint64)[None, :]
        words = philox4x32_10(counter, key).astype(np.uint64).reshape(B, 16)   # block-major: word 4 b + w
        e = ((words[:, 0] * np.uint64(nnz_seq)) >> np.uint64(32)).astype(np.int64)
        u = np.clip(seq_upos[e], 0, nu - 1)
        i = seq_ipos[e]
        start = np.minimum(np.maximum(seq_offsets[u], 0), e)
        c = np.minimum(e - start, window)
        lo = np.clip(row_offsets[u], 0, nnz_seen)
        hi = np.clip(row_offsets[u + 1], lo, nnz_seen)
        j = np.zeros(B, np.int64)
        valid = np.zeros(B, bool)
        for n in range(MAX_TRIES):
            cand = ((words[:, n + 1] * np.uint64(ni)) >> np.uint64(32)).astype(np.int64)
            j = np.where(valid, j, cand)                                      # the last candidate stays when all are seen
            valid = valid | ~bref._row_has(row_ipos, lo, hi, cand)
        for n, a in enumerate((u, e, c, i, j, valid)):
            out[n, k] = a
    return tuple(out) + ((out[5] == 0).sum(1).astype(np.int32),)


# ---- one step --------------------------------------------------------------------------------------------------------------
def context_ids(seq_ipos, e, c):
    """(ids int64[B, 8], mask bool[B, 8]): column n of slot t is seq_ipos[e - c + n] where n < c"""
    seq_ipos, e, c = np.asarray(seq_ipos, np.int64), np.asarray(e, np.int64), np.asarray(c, np.int64)
    n = np.arange(MAX_WINDOW)[None, :]
    mask = n < c[:, None]
    at = np.where(mask, (e - c)[:, None] + n, 0)
    return np.where(mask, seq_ipos[np.clip(at, 0, seq_ipos.size - 1)], 0), mask


def fwd_bwd_ref(user, item, nxt, prev, seq_ipos, u, e, c, i, j, valid, reg, dtype):
    """(loss_t [B], d [B], grads [5 B + M, D], ctx_ids int32[M]) in `dtype`, M = sum of c: the rows [U ; A_i ; A_j ; Bn_i ;
    Bn_j ; context occurrences], occurrence n of slot t at 5 B + (exclusive scan of c)[t] + n.  valid == 0 gives zeros
    under the real ids; a slot with a position outside its table (or an (e, c) that does not stand) gives zeros, and 0 for
    every id that was refused."""
    U, A, Bn, P = (np.asarray(a).astype(dtype) for a in (user, item, nxt, prev))
    u, e, c, i, j = (np.asarray(a, np.int64) for a in (u, e, c, i, j))
    B, nu, ni, nnz = u.size, U.shape[0], A.shape[0], len(seq_ipos)
    stands = (e >= 0) & (e < nnz) & (c >= 0) & (c <= MAX_WINDOW) & (c <= e)
    ce = np.where(stands, c, 0)
    L, mask = context_ids(seq_ipos, np.where(stands, e, 0), ce)
    inside = (L >= 0) & (L < ni)
    bad = ~stands | (mask & ~inside).any(1) | (u < 0) | (u >= nu) | (i < 0) | (i >= ni) | (j < 0) | (j >= ni)
    L = np.where(mask & inside, L, 0)
    ok = ~bad & (np.ones(B, bool) if valid is None else np.asarray(valid) != 0)
    x, ai, aj = U[np.where(ok, u, 0)], A[np.where(ok, i, 0)], A[np.where(ok, j, 0)]
    bi, bj = Bn[np.where(ok, i, 0)], Bn[np.where(ok, j, 0)]
    w = (dtype(1) / np.maximum(ce, 1).astype(dtype))[:, None]
    m = np.zeros_like(x)
    for n in range(MAX_WINDOW):                                                # the chain, oldest first
        m = m + np.where(mask[:, n:n + 1], w * P[L[:, n]], dtype(0))
    da, db = ai - aj, bi - bj
    d = np.sum(x * da, axis=1, dtype=dtype) + np.sum(m * db, axis=1, dtype=dtype)
    loss_t = bref.softplus_neg(d)
    g = bref.sigmoid_neg(d)[:, None]
    reg = dtype(reg)
    gm = -(g * db)
    keep = ok.astype(dtype)
    rows = [reg * x - g * da, reg * ai - g * x, reg * aj + g * x, reg * bi - g * m, reg * bj + g * m]
    five = np.concatenate(rows).astype(dtype) * np.tile(keep, 5)[:, None]
    # the context occurrences, slot-major: the scan of the c handed in (a refused slot keeps its range, as zeros under id 0)
    slot, n = np.nonzero(np.arange(MAX_WINDOW)[None, :] < np.clip(c, 0, MAX_WINDOW)[:, None])
    real = mask[slot, n]
    ctx = (w[slot] * gm[slot] + reg * P[L[slot, n]]).astype(dtype) * (keep[slot] * real)[:, None]
    ctx_ids = np.where(real, L[slot, n], 0).astype(np.int32)
    return loss_t * keep, d * keep, np.concatenate([five, ctx.reshape(-1, U.shape[1])]), ctx_ids


def step_ref(tables, accums, seq_ipos, u, e, c, i, j, valid, reg, lr, optimizer, dtype, eps=EPS):
    """One whole step in `dtype` on the tables / accumulators (dicts over TABLES): a dict with loss_t, d, grads, ctx_ids,
    loss (the mean over the valid slots) and the tables ("user", ...) and accumulators ("user_acc", ...) after the update
    (oracle.optim's row-sparse Adagrad, or the same segment sums applied as SGD)."""
    loss_t, d, grads, ctx_ids = fwd_bwd_ref(*[tables[k] for k in TABLES], seq_ipos, u, e, c, i, j, valid, reg, dtype)
    B = len(u)
    n_valid = B if valid is None else int((np.asarray(valid) != 0).sum())
    ij = np.concatenate([np.asarray(i, np.int64), np.asarray(j, np.int64)])
    parts = {"user": (np.asarray(u, np.int64), grads[:B]), "item": (ij, grads[B:3 * B]), "next": (ij, grads[3 * B:5 * B]),
             "prev": (ctx_ids.astype(np.int64), grads[5 * B:])}
    out = {"loss_t": loss_t, "d": d, "grads": grads, "ctx_ids": ctx_ids,
           "loss": float(np.sum(loss_t, dtype=np.float64)) / n_valid if n_valid else float("nan")}
    for k in TABLES:
        T, Ta = np.asarray(tables[k]).astype(dtype), np.asarray(accums[k]).astype(dtype)
        ids, rows = parts[k]
        if ids.size and optimizer == "adagrad":
            T, Ta = o_optim.sparse_adagrad_update(T, Ta, ids, rows, lr, eps, dtype=dtype)
        elif ids.size:
            T = T.copy()
            uniq, summed = o_optim.segment_sum_rows(ids, rows, dtype)
            T[uniq] = T[uniq] - dtype(lr) * summed
        out[k], out[k + "_acc"] = T, Ta
    return out


# ---- the planted chain of the learning tests -------------------------------------------------------------------------------
PLANTED = dict(nu=200, ni=64, length=20, follow=0.9, rank=8, batch=256, steps=300, window=1, seed=3, k=10)


def planted_sequences():
    """(indices int64, doc_offsets int64[nu + 1]): 200 users of 20 events over 64 items; an event's successor is item
    i + 1 mod 64 with probability 0.9 and a uniform item otherwise -- a first-order structure no set model can see."""
    rng = np.random.default_rng(0)
    nu, ni, length = PLANTED["nu"], PLANTED["ni"], PLANTED["length"]
    seqs = np.zeros((nu, length), np.int64)
    seqs[:, 0] = rng.integers(0, ni, nu)
    for t in range(1, length):
        jump = rng.random(nu) >= PLANTED["follow"]
        seqs[:, t] = np.where(jump, rng.integers(0, ni, nu), (seqs[:, t - 1] + 1) % ni)
    return seqs.reshape(-1), np.arange(nu + 1, dtype=np.int64) * length


def split_last_ref(indices, doc_offsets, n_last=1, min_length=3):
    """evaluate.split_last restated: (context, context_offsets, truth, truth_offsets, kept)"""
    ctx, truth, co, to, kept = [], [], [0], [0], []
    for d in range(len(doc_offsets) - 1):
        doc = list(indices[doc_offsets[d]:doc_offsets[d + 1]])
        if len(doc) >= min_length:
            ctx += doc[:-n_last]
            truth += doc[-n_last:]
            co.append(len(ctx))
            to.append(len(truth))
            kept.append(d)
    return (np.array(ctx, np.int32), np.array(co, np.int64), np.array(truth, np.int32), np.array(to, np.int64),
            np.array(kept, np.int64))


def planted_hit_rate(dtype=np.float64, optimizer="adagrad"):
    """The next-item hit rate@10 under split_last of the reference loop on the planted chain (sample_ref + step_ref for
    PLANTED["steps"] steps; every item is a candidate, seen ones too), and the mean loss of every step."""
    indices, offsets = planted_sequences()
    train, train_off, truth, _, _ = split_last_ref(indices, offsets)
    nu, ni, rank, B = PLANTED["nu"], PLANTED["ni"], PLANTED["rank"], PLANTED["batch"]
    seqs = {u: train[train_off[u]:train_off[u + 1]].tolist() for u in range(nu)}      # (every item occurs: ids are positions)
    (so, su, si), (ro, ri) = seq_csr(seqs, nu)
    rng = np.random.default_rng(1)
    tables = {k: rng.standard_normal((nu if k == "user" else ni, rank)) * rank ** -0.5 for k in TABLES}
    accums = {k: np.full_like(v, ACC0) for k, v in tables.items()}
    losses = []
    for k0 in range(0, PLANTED["steps"], 50):
        draw = sample_ref(so, su, si, ro, ri, nu, ni, PLANTED["window"], PLANTED["seed"], k0, 50, B)
        for k in range(50):
            r = step_ref(tables, accums, si, *[a[k] for a in draw[:6]], REG, LR, optimizer, dtype)
            tables = {key: r[key] for key in TABLES}
            accums = {key: r[key + "_acc"] for key in TABLES}
            losses.append(r["loss"])
    last = np.array([seqs[u][-1] for u in range(nu)])
    scores = tables["user"] @ tables["item"].T + tables["prev"][last] @ tables["next"].T
    top = np.argsort(-scores, axis=1, kind="stable")[:, :PLANTED["k"]]
    return float((top == truth[:, None]).any(1).mean()), losses

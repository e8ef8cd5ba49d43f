"""Plain NumPy reference of Bayesian Personalised Ranking as esr_bpr.hip and factorization.BPR compute it: the triple
sampler of esr_bpr_sample.h restated line by line, one step (per-triple loss, score difference, gradient rows, row-sparse
Adagrad or SGD on both tables through oracle.optim), the planted corpus of the learning tests and the tolerance rule.  No
GPU, no torch: tests/test_bpr_ref.py checks all of it on the CPU, tests/test_gpu_bpr.py runs the kernels against it.

The tolerance rule is the one of the one-pass steps (tests/_triplet_step_ref.py):

    kernel error against fp64  <=  FACTOR * e32 + 2^-22,   e32 = error of the SAME restatement run in float32 against fp64

(arrays: max |a - b| / max |b|, what conftest.rel_err computes; the loss of a step: relative difference).  FACTOR = 4, the
factor of that module, for its reason: the kernel's dot product is four fmaf per lane and a butterfly over the lanes, NumPy
sums pairwise -- two f32 evaluations in other association orders -- and a gradient row's segment sum runs left to right in
both.  The device's expf / log1pf are precise forms (a few ulp) and do not make 4 too tight on loss_t: measured on an
MI355X (profiles/bpr/parity_errors.json and README.md) the kernel's error on loss_t is at most 1.4 times e32 and 0.16 of
the bound, on d 2.1 times and 0.25, on the gradient rows 1.3 times and 0.23.  The factor stays 4.
"""
import numpy as np

from _spotify_sampler_ref import philox4x32_10
from oracle import optim as o_optim

MAX_TRIES = 15
FLOOR = 2.0 ** -22
FACTOR = 4.0
LR, EPS, REG, ACC0 = 0.05, 1e-7, 0.01, 0.1
ARRAYS = ("loss_t", "d", "grads", "user", "item", "user_acc", "item_acc")


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def _row_has(row_ipos, lo, hi, j):
    """bpr_row_has for arrays of (lo, hi, j): the 32-probe lower bound, then the comparison"""
    lo, hi, end = lo.copy(), hi.copy(), hi.copy()
    safe = np.concatenate([row_ipos, [0]]).astype(np.int64)
    for _ in range(32):
        live = lo < hi
        mid = lo + ((hi - lo) >> 1)
        less = live & (safe[np.minimum(mid, row_ipos.size)] < j)
        lo = np.where(less, mid + 1, lo)
        hi = np.where(live & ~less, mid, hi)
    return (lo < end) & (safe[np.minimum(lo, row_ipos.size)] == j)


def sample_ref(row_offsets, row_upos, row_ipos, nu, ni, seed, step0, K, B):
    """(u, i, j, valid) int32 [K, B] and dropped int32[K] by the rule of esr_bpr_sample.h."""
    row_offsets, row_upos, row_ipos = (np.asarray(a, np.int64) for a in (row_offsets, row_upos, row_ipos))
    nnz = row_upos.size
    assert 1 <= nnz <= 2 ** 31 - 1 and 1 <= ni <= 2 ** 31 - 1 and row_offsets.size == nu + 1
    seed = int(seed) & (2 ** 64 - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    out = np.zeros((4, K, B), np.int32)
    t = np.arange(B, dtype=np.uint64)
    for k in range(K):
        s = (int(step0) + k) & 0xFFFFFFFF
        counter = np.zeros((B, 4, 4), np.uint64)          # [slot, block, counter word] = (t, s, b, 0)
        counter[:, :, 0] = t[:, None]
        counter[:, :, 1] = s
        counter[:, :, 2] = np.arange(4, dtype=np.uint64)[None, :]
        words = philox4x32_10(counter, key).astype(np.uint64).reshape(B, 16)   # block-major: word 4 b + w
        p = ((words[:, 0] * np.uint64(nnz)) >> np.uint64(32)).astype(np.int64)
        u = np.clip(row_upos[p], 0, nu - 1)
        i = row_ipos[p]
        lo = np.clip(row_offsets[u], 0, nnz)
        hi = np.clip(row_offsets[u + 1], lo, nnz)
        j = np.zeros(B, np.int64)
        valid = np.zeros(B, bool)
        for c in range(MAX_TRIES):
            cand = ((words[:, c + 1] * np.uint64(ni)) >> np.uint64(32)).astype(np.int64)
            j = np.where(valid, j, cand)                                      # the last candidate stays when all are seen
            valid = valid | ~_row_has(row_ipos, lo, hi, cand)
        out[0, k], out[1, k], out[2, k], out[3, k] = u, i, j, valid
    return out[0], out[1], out[2], out[3], (out[3] == 0).sum(1).astype(np.int32)


def csr_of(rows, nu):
    """(row_offsets int64[nu + 1], row_upos, row_ipos int32) of {user position: iterable of item positions}"""
    upos, ipos, off = [], [], [0]
    for u in range(nu):
        items = sorted(set(rows.get(u, ())))
        upos += [u] * len(items)
        ipos += items
        off.append(len(upos))
    return np.array(off, np.int64), np.array(upos, np.int32), np.array(ipos, np.int32)


def random_csr(rng, nu, ni, lengths):
    """a CSR whose row r holds lengths[r % len(lengths)] distinct item positions (at most ni)"""
    return csr_of({u: rng.choice(ni, min(ni, lengths[u % len(lengths)]), replace=False).tolist() for u in range(nu)}, nu)


# ---- one step --------------------------------------------------------------------------------------------------------------
def softplus_neg(d):
    """softplus(-d) = max(-d, 0) + log1p(exp(-|d|)) in d's dtype"""
    return np.maximum(-d, 0) + np.log1p(np.exp(-np.abs(d)))


def sigmoid_neg(d):
    """sigmoid(-d) from exp(-|d|): neither branch overflows"""
    e = np.exp(-np.abs(d))
    return np.where(d >= 0, e, np.ones_like(e)) / (1 + e)


def fwd_bwd_ref(user, item, u, i, j, valid, reg, dtype):
    """(loss_t [B], d [B], grads [3 B, D]) in `dtype`; ids outside a table and valid == 0 give zeros."""
    U, Y = np.asarray(user).astype(dtype), np.asarray(item).astype(dtype)
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    B = u.size
    ok = np.ones(B, bool) if valid is None else np.asarray(valid) != 0
    ok = ok & (u >= 0) & (u < U.shape[0]) & (i >= 0) & (i < Y.shape[0]) & (j >= 0) & (j < Y.shape[0])
    x, yi, yj = U[np.where(ok, u, 0)], Y[np.where(ok, i, 0)], Y[np.where(ok, j, 0)]
    d = np.sum(x * (yi - yj), axis=1, dtype=dtype)
    loss_t = softplus_neg(d)
    g = sigmoid_neg(d)[:, None]
    reg = dtype(reg)
    grads = np.concatenate([-g * (yi - yj) + reg * x, -g * x + reg * yi, g * x + reg * yj]).astype(dtype)
    keep = ok.astype(dtype)
    return loss_t * keep, d * keep, grads * np.tile(keep, 3)[:, None]


def step_ref(user, item, user_acc, item_acc, u, i, j, valid, reg, lr, optimizer, dtype, eps=EPS):
    """One whole step in `dtype`: a dict with loss_t, d, grads, loss (the mean over the valid triples) and the tables and
    accumulators after the update (oracle.optim's row-sparse Adagrad, or the same segment sums applied as SGD)."""
    loss_t, d, grads = fwd_bwd_ref(user, item, u, i, j, valid, reg, dtype)
    B = len(u)
    n_valid = B if valid is None else int((np.asarray(valid) != 0).sum())
    U, Y = np.asarray(user).astype(dtype), np.asarray(item).astype(dtype)
    Ua, Ya = np.asarray(user_acc).astype(dtype), np.asarray(item_acc).astype(dtype)
    ij = np.concatenate([np.asarray(i, np.int64), np.asarray(j, np.int64)])
    if optimizer == "adagrad":
        U, Ua = o_optim.sparse_adagrad_update(U, Ua, u, grads[:B], lr, eps, dtype=dtype)
        Y, Ya = o_optim.sparse_adagrad_update(Y, Ya, ij, grads[B:], lr, eps, dtype=dtype)
    else:
        for table, ids, rows in ((U, u, grads[:B]), (Y, ij, grads[B:])):
            uniq, summed = o_optim.segment_sum_rows(ids, rows, dtype)
            table[uniq] = table[uniq] - dtype(lr) * summed
    loss = float(np.sum(loss_t, dtype=np.float64)) / n_valid if n_valid else float("nan")
    return {"loss_t": loss_t, "d": d, "grads": grads, "loss": loss, "user": U, "item": Y, "user_acc": Ua, "item_acc": Ya}


def arr_err(a, b):
    """max |a - b| / max |b|  (conftest.rel_err without its log)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30)) if a.size else 0.0


def bounds(r32, r64, keys):
    """{quantity: FACTOR * e32 + 2^-22} and the e32 themselves"""
    e32 = {k: arr_err(r32[k], r64[k]) for k in keys}
    return {k: FACTOR * v + FLOOR for k, v in e32.items()}, e32


# ---- the planted corpus of the learning tests ---------------------------------------------------------------------------
PLANTED = dict(nu=64, ni=64, per_user=8, rank=8, batch=256, steps=60, seed=3)


def planted_pairs(rng=None):
    """(user, item) int64: 64 users, 64 items, two communities -- every user has seen 8 items of its own half."""
    rng = np.random.default_rng(0) if rng is None else rng
    nu, ni, per = PLANTED["nu"], PLANTED["ni"], PLANTED["per_user"]
    user = np.repeat(np.arange(nu), per)
    item = np.concatenate([rng.choice(ni // 2, per, replace=False) + (ni // 2) * (u >= nu // 2) for u in range(nu)])
    return user.astype(np.int64), item.astype(np.int64)


def planted_losses(dtype=np.float64, optimizer="adagrad"):
    """The mean loss of each of the 60 steps of the reference loop on the planted corpus (sample_ref + step_ref)."""
    user, item = planted_pairs()
    nu, ni, rank, B = PLANTED["nu"], PLANTED["ni"], PLANTED["rank"], PLANTED["batch"]
    off, upos, ipos = csr_of({u: item[user == u].tolist() for u in range(nu)}, nu)
    rng = np.random.default_rng(1)
    U, Y = rng.standard_normal((nu, rank)) * rank ** -0.5, rng.standard_normal((ni, rank)) * rank ** -0.5
    Ua, Ya = np.full_like(U, ACC0), np.full_like(Y, ACC0)
    losses = []
    u, i, j, valid, _ = sample_ref(off, upos, ipos, nu, ni, PLANTED["seed"], 0, PLANTED["steps"], B)
    for k in range(PLANTED["steps"]):
        r = step_ref(U, Y, Ua, Ya, u[k], i[k], j[k], valid[k], REG, LR, optimizer, dtype)
        U, Y, Ua, Ya = r["user"], r["item"], r["user_acc"], r["item_acc"]
        losses.append(r["loss"])
    return losses

"""Plain NumPy reference of the WARP step as esr_warp.hip and factorization.WARP compute it: the rule of
esr_warp_sample.h restated over all slots at once in a chosen dtype (the Philox stream and the row search are those of
tests/_bpr_ref.py; scores are taken with np.sum), one whole step through oracle.optim, the cases the CPU and GPU tests
share, the planted corpus of tests/_bpr_ref.py and its tolerance rule.  No GPU, no torch.

Two kinds of tables.
  Exact: entries that are multiples of 2^-6 in [-2, 2], margin, reg and rank_weight multiples of 2^-6.  At D <= 128 every
    product and partial sum of a score is exact in float32 (|sum| < 2^21 * 2^-12), so any summation order gives the same
    bits and the fp64 restatement is the truth: the kernel and the host program must equal it bit for bit (the loss and the
    gradient entries are exact in fp64 and rounded once, as one float32 operation -- fused or not -- rounds them).  Ties
    d == margin are planted.
  Random: randn * scale.  The selection of a slot can turn on the last bits of a score, so a slot is *undecided* when some
    scored candidate has |d64 - margin| <= 2^-18 (sum |x| |y_i| + sum |x| |y_j|) -- 64 float32 epsilons of the terms'
    size, far more than any summation order of <= 128 terms moves d.  Undecided slots are left out of the selection
    comparison; they may be at most UNDECIDED_CAP = 1 % of a case's slots (a condition on the cases, not a measurement).

The tolerance rule over the slots whose selection agrees is that of _bpr_ref:

    kernel error against fp64  <=  FACTOR * e32 + 2^-22,   e32 = error of the SAME restatement run in float32 against fp64

with FACTOR = 4 for the reason given there: the kernel's dot product is four fmaf per lane and a butterfly over the lanes,
NumPy sums pairwise -- two float32 evaluations in other association orders.

The planted corpus.  planted_run(np.float64) -- 60 steps of step_ref on _bpr_ref.PLANTED from the factors
factorization.WARP draws for seed 3 (PLANTED_WARP below: max_trials 16, margin 1, harmonic weights, Adagrad) -- reaches
auc 0.8789 (from 0.5430 before training) over the 256 triples BPR's sampler draws under seed 4, step 0; its mean trials
per slot rise from 1.023 at step 0 to 2.199 at step 59.
"""
import numpy as np

import _bpr_ref as bref
from _bpr_ref import FACTOR, FLOOR, arr_err, bounds, csr_of, random_csr  # noqa: F401  (the tests take them from here)
from _spotify_sampler_ref import philox4x32_10
from oracle import optim as o_optim

MAX_TRIALS = 255
UNDECIDED_CAP = 0.01
UNDECIDED_WINDOW = 2.0 ** -18
IDS = ("u", "i", "j", "valid", "trials")
ARRAYS = ("loss_t", "d", "grads")


# ---- the rule --------------------------------------------------------------------------------------------------------------
def _slot_numbers(B, slots):
    """the slot numbers a restatement runs over: arange(B), or the chosen ones (each in [0, B))"""
    if slots is None:
        return np.arange(B, dtype=np.int64)
    slots = np.asarray(slots, np.int64).reshape(-1)
    assert slots.size == 0 or (0 <= slots.min() and slots.max() < B)
    return slots


def stream_words(seed, step, B, nwords, slots=None):
    """uint64 [B, >= nwords]: word 4 b + w of slot t is word w of philox4x32_10((t, step, b, 0), (seed lo, seed hi)); with
    `slots` (int array of slot numbers below B) row n is the stream of slot slots[n]"""
    seed = int(seed) & (2 ** 64 - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    nblocks = (nwords + 3) // 4
    slots = _slot_numbers(B, slots)
    B = slots.size
    counter = np.zeros((B, nblocks, 4), np.uint64)
    counter[:, :, 0] = slots.astype(np.uint64)[:, None]
    counter[:, :, 1] = int(step) & 0xFFFFFFFF
    counter[:, :, 2] = np.arange(nblocks, dtype=np.uint64)[None, :]
    return philox4x32_10(counter, key).astype(np.uint64).reshape(B, 4 * nblocks)


def harmonic(ni):
    return np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, ni + 1, dtype=np.float64))]).astype(np.float32)


def warp_ref(user, item, csr, rank_weight, seed, step, B, T, margin, reg, dtype, slots=None):
    """The step's outputs by the rule of esr_warp_sample.h in `dtype`: a dict with u, i, j, valid, trials (int32 [B]), s_i,
    d, loss_t ([B]), grads ([3 B, D]), bad (did a slot meet an item position outside the table) and undecided (bool [B]:
    some scored candidate lies within the window around the margin; meaningful for dtype = float64).  With `slots` (an
    int array of slot numbers below B) the rule runs for those slots only: every output is indexed by the position in
    `slots` and grads is [3 len(slots), D] -- a slot is a function of its own number, never of B."""
    row_offsets, row_upos, row_ipos = (np.asarray(a, np.int64) for a in csr)
    U, Y = np.asarray(user).astype(dtype), np.asarray(item).astype(dtype)
    nu, ni, nnz, D = U.shape[0], Y.shape[0], row_upos.size, U.shape[1]
    assert 1 <= T <= MAX_TRIALS and row_offsets.size == nu + 1 and np.asarray(rank_weight).shape == (ni + 1,)
    weight = np.asarray(rank_weight, np.float32).astype(dtype)
    margin, reg = dtype(np.float32(margin)), dtype(np.float32(reg))
    words = stream_words(seed, step, B, T + 1, slots)
    B = words.shape[0]
    p = ((words[:, 0] * np.uint64(nnz)) >> np.uint64(32)).astype(np.int64)
    u = np.clip(row_upos[p], 0, nu - 1)
    i = row_ipos[p]
    lo = np.clip(row_offsets[u], 0, nnz)
    hi = np.clip(row_offsets[u + 1], lo, nnz)
    bad = (i < 0) | (i >= ni)
    x, yi = U[u], Y[np.where(bad, 0, i)]
    absx = np.abs(x).astype(np.float64)
    s_i = np.sum(x * yi, axis=1, dtype=dtype)
    size_i = np.sum(absx * np.abs(yi), axis=1)
    j, trials = np.zeros(B, np.int64), np.zeros(B, np.int64)
    valid, undecided, d = np.zeros(B, bool), np.zeros(B, bool), np.zeros(B, dtype)
    yj = yi.copy()
    for c in range(T):
        walking = ~valid & ~bad
        if not walking.any():
            break
        cand = ((words[:, c + 1] * np.uint64(ni)) >> np.uint64(32)).astype(np.int64)
        j = np.where(walking, cand, j)
        scored = walking & ~bref._row_has(row_ipos, lo, hi, cand)
        trials += scored
        yc = Y[cand]
        dc = s_i - np.sum(x * yc, axis=1, dtype=dtype)
        near = np.abs(dc.astype(np.float64) - float(margin)) <= UNDECIDED_WINDOW * (size_i + np.sum(absx * np.abs(yc), axis=1))
        undecided |= scored & near
        hit = scored & (dc < margin)
        d = np.where(hit, dc, d)
        yj[hit] = yc[hit]
        valid |= hit
    r = np.maximum(1, (ni - (hi - lo)) // np.maximum(trials, 1))
    w = np.where(valid, weight[np.clip(r, 0, ni)], 0).astype(dtype)
    loss_t = w * (margin - d) * valid
    wc, keep = w[:, None], valid[:, None].astype(dtype)
    grads = np.concatenate([(reg * x - wc * (yi - yj)) * keep, (reg * yi - wc * x) * keep, (reg * yj + wc * x) * keep])
    return {"u": u.astype(np.int32), "i": i.astype(np.int32), "j": j.astype(np.int32), "valid": valid.astype(np.int32),
            "trials": trials.astype(np.int32), "s_i": s_i * ~bad, "d": d, "loss_t": loss_t.astype(dtype),
            "grads": grads.astype(dtype), "bad": bool(bad.any()), "undecided": undecided}


def same_selection(a, b):
    """bool [B]: the slots on which two results took the same (u, i, j, valid, trials)"""
    return np.logical_and.reduce([np.asarray(a[k]) == np.asarray(b[k]) for k in IDS])


def slot_rows(mask):
    """the mask of a slot set over the 3 B gradient rows"""
    return np.tile(mask, 3)


def restrict(r, mask):
    return {"loss_t": r["loss_t"][mask], "d": r["d"][mask], "grads": r["grads"][slot_rows(mask)]}


def step_ref(user, item, user_acc, item_acc, csr, rank_weight, seed, step, B, T, margin, reg, lr, optimizer, dtype,
             eps=bref.EPS):
    """One whole step in `dtype`: warp_ref's outputs, loss (the mean over the valid slots, NaN without one), mean_trials and
    the tables and accumulators after the update (oracle.optim's row-sparse Adagrad, or the same segment sums as SGD)."""
    r = warp_ref(user, item, csr, rank_weight, seed, step, B, T, margin, reg, dtype)
    U, Y = np.asarray(user).astype(dtype), np.asarray(item).astype(dtype)
    Ua, Ya = np.asarray(user_acc).astype(dtype), np.asarray(item_acc).astype(dtype)
    u, grads = r["u"].astype(np.int64), r["grads"]
    ij = np.concatenate([r["i"], r["j"]]).astype(np.int64)
    if optimizer == "adagrad":
        U, Ua = o_optim.sparse_adagrad_update(U, Ua, u, grads[:B], lr, eps, dtype=dtype)
        Y, Ya = o_optim.sparse_adagrad_update(Y, Ya, ij, grads[B:], lr, eps, dtype=dtype)
    else:
        for table, ids, rows in ((U, u, grads[:B]), (Y, ij, grads[B:])):
            uniq, summed = o_optim.segment_sum_rows(ids, rows, dtype)
            table[uniq] = table[uniq] - dtype(lr) * summed
    n = int(r["valid"].sum())
    r.update(loss=float(np.sum(r["loss_t"], dtype=np.float64)) / n if n else float("nan"),
             mean_trials=float(r["trials"].sum()) / B, user=U, item=Y, user_acc=Ua, item_acc=Ya)
    return r


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------
EXACT_D = (4, 8, 32, 64, 100, 128)
EXACT_B = (1, 63, 64, 65, 257)
EXACT_T = (1, 3, 4, 5, 16, 255)
EXACT_REG = 2.0 ** -6
_CACHE = {}


def exact_tables(rng, nu, ni, D):
    """float32 tables whose entries are multiples of 2^-6 in [-2, 2]"""
    return ((rng.integers(-128, 129, (nu, D)) / 64.0).astype(np.float32),
            (rng.integers(-128, 129, (ni, D)) / 64.0).astype(np.float32))


def exact_weights(rng, ni):
    """rank weights that are multiples of 2^-6 in [0, 4), entry 0 = 0"""
    w = (rng.integers(0, 256, ni + 1) / 64.0).astype(np.float32)
    w[0] = 0
    return w


def _case(name, U, Y, csr, weight, seed, step, B, T, margin, reg):
    return dict(name=name, user=U, item=Y, csr=csr, weight=weight, seed=seed, step=step, B=B, T=T, margin=np.float32(margin),
                reg=np.float32(reg))


def exact_grid_cases(D):
    """the grid of one rank: every B and T on one pair of exact tables; the margin of a T is the multiple of 2^-6 next to
    the min(1 / 2, 2 / T) quantile of d over the pairs, so that searches end at every trial count up to T"""
    rng = np.random.default_rng([7, D])
    nu, ni = 23, 97
    U, Y = exact_tables(rng, nu, ni, D)
    csr = random_csr(rng, nu, ni, (1, 3, 17, 40))
    weight = exact_weights(rng, ni)
    s = U.astype(np.float64) @ Y.astype(np.float64).T
    spread = (s[:, :, None] - s[:, None, :])[:, :16, :].reshape(-1)
    for T in EXACT_T:
        margin = np.round(np.quantile(spread, min(0.5, 2.0 / T)) * 64) / 64
        for B in EXACT_B:
            yield _case("grid-D%d-B%d-T%d" % (D, B, T), U, Y, csr, weight, (0xC0FFEE << 32) | (D * 1000 + T), 17 + B, B, T,
                        margin, EXACT_REG)


def exact_planted_cases():
    rng = np.random.default_rng(8)
    out = []
    # a user who has seen every item: no unseen candidate, valid = 0 and trials = 0; the other user has seen one
    U, Y = exact_tables(rng, 2, 12, 8)
    out.append(_case("seen-everything", U, Y, csr_of({0: range(12), 1: [5]}, 2), exact_weights(rng, 12), 5, 0, 257, 16, 0.5,
                     EXACT_REG))
    # a user who has seen all but one of 1024 items: most searches meet no unseen candidate, r = 1 / N = 1
    U, Y = exact_tables(rng, 1, 1024, 32)
    Y[77] = np.where(U[0] >= 0, 2.0, -2.0)                          # the one unseen item outscores any positive: d <= 0
    out.append(_case("all-but-one", U, Y, csr_of({0: [k for k in range(1024) if k != 77]}, 1), exact_weights(rng, 1024), 6, 3,
                     257, 255, 1.0, EXACT_REG))
    # ni = 1: the item is seen
    U, Y = exact_tables(rng, 2, 1, 4)
    out.append(_case("one-item", U, Y, csr_of({0: [0], 1: []}, 2), exact_weights(rng, 1), 7, 0, 65, 5, 1.0, EXACT_REG))
    # planted ties: one user, items whose scores against it are s, s - margin (d == margin: NOT a violation) and
    # s - margin + 2^-6 (the smallest violation): rows with a single nonzero entry
    D, ni, margin = 16, 40, 0.75
    U = np.zeros((1, D), np.float32)
    U[0, 3] = 1.0
    Y = np.zeros((ni, D), np.float32)
    Y[:, 5] = (rng.integers(-128, 129, ni) / 64.0)
    Y[0, 3] = 1.5                                                   # the positive
    Y[1:30, 3] = 1.5 - margin                                       # ties
    Y[30:, 3] = 1.5 - margin + 2.0 ** -6                            # violators: d = margin - 2^-6
    out.append(_case("ties", U, Y, csr_of({0: [0]}, 1), exact_weights(rng, ni), 9, 1, 257, 16, margin, EXACT_REG))
    # exactly one item violates (1 in 64): the groups of one wave end at trial 1 and at trial T side by side
    D, ni = 64, 64
    U, Y = exact_tables(rng, 4, ni, D)
    U = np.abs(U) + np.float32(2.0 ** -6)                           # every user row is positive ...
    Y[:9] *= 0                                                      # ... the seen items (and item 0) score 0: ties at best ...
    Y[9:] = np.float32(-2.0)                                        # ... every other item scores far below them ...
    Y[40] = np.float32(2.0)                                         # ... but one
    out.append(_case("one-violator", U, Y, csr_of({k: [1 + 2 * k, 2 + 2 * k] for k in range(4)}, 4), exact_weights(rng, ni), 10,
                     2, 257, 16, 0.0, 0.0))
    return out


def exact_cases():
    """every exact case with its fp64 reference, computed once: [(case, reference)]"""
    if "exact" not in _CACHE:
        cases = [c for D in EXACT_D for c in exact_grid_cases(D)] + exact_planted_cases()
        _CACHE["exact"] = [(c, reference(c, np.float64)) for c in cases]
    return _CACHE["exact"]


def random_tables(rng, nu, ni, D, scale=None):
    """rows of size D^(-1/4) per element: a score difference is of order 1"""
    s = D ** -0.25 if scale is None else scale
    return (rng.standard_normal((nu, D)) * s).astype(np.float32), (rng.standard_normal((ni, D)) * s).astype(np.float32)


def random_case_list():
    out = []
    for D, B, T, margin, scale in ((8, 257, 4, 1.0, None), (64, 1024, 32, 1.0, None), (100, 257, 32, 0.5, None),
                                   (128, 300, 16, 1.0, None), (32, 257, 255, -2.0, None), (4, 65, 3, 0.25, None)):
        rng = np.random.default_rng([9, D, T])
        nu, ni = 37, 211
        U, Y = random_tables(rng, nu, ni, D, scale)
        out.append(_case("random-D%d-B%d-T%d" % (D, B, T), U, Y, random_csr(rng, nu, ni, (1, 2, 20, 63, 64, 65)), harmonic(ni),
                         (0xBEEF << 32) | D, 2 ** 32 - 1 if D == 8 else T, B, T, margin, 0.01))
    return out


def random_cases():
    """[(case, fp64 reference, float32 reference)], computed once"""
    if "random" not in _CACHE:
        _CACHE["random"] = [(c, reference(c, np.float64), reference(c, np.float32)) for c in random_case_list()]
    return _CACHE["random"]


def reference(case, dtype):
    return warp_ref(case["user"], case["item"], case["csr"], case["weight"], case["seed"], case["step"], case["B"], case["T"],
                    case["margin"], case["reg"], dtype)


# ---- the planted corpus of the learning tests ---------------------------------------------------------------------------
PLANTED = bref.PLANTED
PLANTED_WARP = dict(max_trials=16, margin=1.0)
planted_pairs = bref.planted_pairs


def planted_csr():
    user, item = planted_pairs()
    return csr_of({u: item[user == u].tolist() for u in range(PLANTED["nu"])}, PLANTED["nu"])


def auc_ref(U, Y, csr, nu, ni, seed, B):
    """BPR.auc(K = 1): the share of the valid triples of bpr_sample(seed, step 0) with d > 0, a tie counting half"""
    u, i, j, valid, _ = bref.sample_ref(*csr, nu, ni, seed, 0, 1, B)
    u, i, j, ok = u[0].astype(np.int64), i[0].astype(np.int64), j[0].astype(np.int64), valid[0] != 0
    d = np.sum(U[u] * (Y[i] - Y[j]), axis=1)
    return float(((d > 0) & ok).sum() + 0.5 * ((d == 0) & ok).sum()) / int(ok.sum())


def planted_run(user0, item0, dtype=np.float64, optimizer="adagrad"):
    """The reference loop on the planted corpus from the given factors: 60 steps of step_ref.  Returns (auc before, auc
    after, the steps' mean trials, the steps' mean losses)."""
    nu, ni, B, seed = PLANTED["nu"], PLANTED["ni"], PLANTED["batch"], PLANTED["seed"]
    csr = planted_csr()
    U, Y = np.asarray(user0).astype(dtype), np.asarray(item0).astype(dtype)
    Ua, Ya = np.full_like(U, bref.ACC0), np.full_like(Y, bref.ACC0)
    before = auc_ref(U, Y, csr, nu, ni, seed + 1, B)
    trials, losses = [], []
    for k in range(PLANTED["steps"]):
        r = step_ref(U, Y, Ua, Ya, csr, harmonic(ni), seed, k, B, PLANTED_WARP["max_trials"], PLANTED_WARP["margin"], bref.REG,
                     bref.LR, optimizer, dtype)
        U, Y, Ua, Ya = r["user"], r["item"], r["user_acc"], r["item_acc"]
        trials.append(r["mean_trials"])
        losses.append(r["loss"])
    return before, auc_ref(U, Y, csr, nu, ni, seed + 1, B), trials, losses

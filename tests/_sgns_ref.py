"""Plain NumPy reference of skip-gram with negative sampling as esr_sgns.hip and factorization.SGNS compute it: the noise
table (integer masses and Walker / Vose alias columns), the slot sampler of esr_sgns_sample.h restated line by line, one
step (per-slot loss, the 1 + K scores, the 2 + K gradient rows in fp64 and in the kernel's float32 chain order, row-sparse
Adagrad or SGD on both tables through oracle.optim), the planted corpus of the learning tests and the tolerance rule.  No
GPU, no torch: tests/test_sgns_ref.py checks all of it on the CPU, tests/test_gpu_sgns.py runs the kernels against it.

The tolerance rule is _bpr_ref's, for its reasons (the kernel's dot product is four fmaf per lane and a butterfly, NumPy
sums pairwise; the centre's gradient row is a chain of 1 + K fmaf against NumPy's multiply and add):

    kernel error against fp64  <=  4 * e32 + 2^-22,   e32 = error of the SAME restatement run in float32 against fp64
"""
import numpy as np

import _bpr_ref as bref
from _spotify_sampler_ref import philox4x32_10
from oracle import optim as o_optim

MAX_WINDOW, MAX_NEGATIVES = 32, 16
COLUMN = 1 << 32
FLOOR, FACTOR = bref.FLOOR, bref.FACTOR
LR, EPS, REG, ACC0 = bref.LR, bref.EPS, bref.REG, bref.ACC0
KEYS = ("loss_t", "s", "centre", "positive", "noise")
arr_err = bref.arr_err
bounds = bref.bounds


# ---- the noise table -----------------------------------------------------------------------------------------------------
def noise_masses(counts, power=0.75):
    """integer masses (python ints) of count ** power that sum to ni * 2^32: floors of the float64 targets, at least 1 for
    an item that occurs, the remainder spread one unit at a time in descending mass (ascending id among equals)"""
    counts = [int(c) for c in counts]
    ni, total = len(counts), len(counts) * COLUMN
    f = np.array([float(c) ** power if c > 0 else 0.0 for c in counts], np.float64)
    raw = f / f.sum() * total
    m = [max(int(np.floor(r)), 1) if c > 0 else 0 for r, c in zip(raw, counts)]
    order = sorted((i for i in range(ni) if counts[i] > 0), key=lambda i: (-m[i], i))
    rest = total - sum(m)
    if rest > 0:
        q, r = divmod(rest, len(order))
        for n, i in enumerate(order):
            m[i] += q + (n < r)
    for i in order:                                                           # (rest < 0: taken from the heaviest first)
        take = min(m[i] - 1, max(-rest, 0))
        m[i] -= take
        rest += take
    assert sum(m) == total
    return m


def alias_table(masses):
    """(keep uint32[ni], alias int32[ni]) of the integer masses by Vose's pairing on exact integers: the lightest open
    column (ascending id) is filled from the heaviest open one (ascending id)"""
    rem = [int(v) for v in masses]
    ni = len(rem)
    keep, alias = [COLUMN - 1] * ni, list(range(ni))
    small = [i for i in reversed(range(ni)) if rem[i] < COLUMN]
    large = [i for i in reversed(range(ni)) if rem[i] > COLUMN]
    while small and large:
        s, l = small.pop(), large.pop()
        keep[s], alias[s] = rem[s], l
        rem[l] -= COLUMN - rem[s]
        (small if rem[l] < COLUMN else large if rem[l] > COLUMN else []).append(l)
    assert not small and not large
    return np.array(keep, np.uint32), np.array(alias, np.int32)


def table_masses(keep, alias):
    """the masses an alias table represents: keep' of every column plus what the other columns hand to it"""
    ni = len(keep)
    full = np.asarray(alias) == np.arange(ni)
    got = [COLUMN if full[n] else int(keep[n]) for n in range(ni)]
    for n in np.nonzero(~full)[0]:
        got[int(alias[n])] += COLUMN - int(keep[n])
    return got


# ---- the sampler ---------------------------------------------------------------------------------------------------------
def doc_csr(docs):
    """(seq_offsets int64[nd + 1], seq_upos, seq_ipos int32) of a list of documents (item positions in order)"""
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    upos = np.repeat(np.arange(len(docs)), [len(d) for d in docs]).astype(np.int32)
    return off, upos, np.array([v for d in docs for v in d], np.int32)


def sample_ref(seq_offsets, seq_upos, seq_ipos, nd, ni, window, K, keep, alias, seed, step0, steps, B):
    """(c, e, o, valid) int32 [steps, B], neg int32 [steps, B, K] and dropped int32[steps] by the rule of esr_sgns_sample.h."""
    seq_offsets, seq_upos, seq_ipos = (np.asarray(a, np.int64) for a in (seq_offsets, seq_upos, seq_ipos))
    keep, alias = np.asarray(keep, np.uint64), np.asarray(alias, np.int64)
    nnz = seq_upos.size
    assert 1 <= nnz <= 2 ** 31 - 1 and 1 <= ni <= 2 ** 31 - 1 and seq_offsets.size == nd + 1
    assert 1 <= window <= MAX_WINDOW and 1 <= K <= MAX_NEGATIVES and keep.size == ni == alias.size
    seed = int(seed) & (2 ** 64 - 1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    out = np.zeros((4, steps, B), np.int32)
    neg = np.zeros((steps, B, K), np.int32)
    t = np.arange(B, dtype=np.uint64)
    nblocks = 1 + (K + 1) // 2
    for k in range(steps):
        s = (int(step0) + k) & 0xFFFFFFFF
        counter = np.zeros((B, nblocks, 4), np.uint64)     # [slot, block, counter word] = (t, s, b, 0)
        counter[:, :, 0] = t[:, None]
        counter[:, :, 1] = s
        counter[:, :, 2] = np.arange(nblocks, dtype=np.uint64)[None, :]
        words = philox4x32_10(counter, key).astype(np.uint64).reshape(B, 4 * nblocks)   # block-major: word 4 b + w
        e = ((words[:, 0] * np.uint64(nnz)) >> np.uint64(32)).astype(np.int64)
        c = seq_ipos[e]
        u = np.clip(seq_upos[e], 0, nd - 1)
        start = np.minimum(np.maximum(seq_offsets[u], 0), e)
        end = np.minimum(np.maximum(seq_offsets[u + 1], e + 1), nnz)
        rem = ((words[:, 1] * np.uint64(window * (window + 1) // 2)) >> np.uint64(32)).astype(np.int64)
        weight, d = np.full(B, window, np.int64), np.ones(B, np.int64)
        going = np.ones(B, bool)
        for _ in range(1, window):                                            # the loop of at most window turns
            going = going & (rem >= weight)
            rem, weight, d = np.where(going, rem - weight, rem), np.where(going, weight - 1, weight), d + going
        p = np.where((words[:, 2] >> np.uint64(31)) != 0, e + d, e - d)
        valid = (p >= start) & (p < end)
        o = np.where(valid, seq_ipos[np.clip(p, 0, nnz - 1)], c)
        for n, a in enumerate((c, e, o, valid)):
            out[n, k] = a
        for j in range(K):
            col = ((words[:, 4 * (1 + (j >> 1)) + 2 * (j & 1)] * np.uint64(ni)) >> np.uint64(32)).astype(np.int64)
            neg[k, :, j] = np.where(words[:, 4 * (1 + (j >> 1)) + 2 * (j & 1) + 1] < keep[col], col, alias[col])
    return out[0], out[1], out[2], out[3], neg, (out[3] == 0).sum(1).astype(np.int32)


DOC_LENGTHS = (1, 2, 3, 5, 6, 33, 1000)


def boundary_corpus():
    """documents of the lengths (1, 2, 3, 5, 6, 33, 1000) over ni = 1001, every item occurring; its noise table"""
    rng = np.random.default_rng(4)
    docs = [rng.integers(0, 1001, n).tolist() for n in DOC_LENGTHS[:-1]] + [rng.permutation(1001)[:1000].tolist()]
    counts = np.bincount(np.concatenate([np.array(d) for d in docs]), minlength=1001)
    keep, alias = alias_table(noise_masses(counts))
    return doc_csr(docs), len(docs), 1001, keep, alias


# ---- one step --------------------------------------------------------------------------------------------------------------
def softplus(s):
    return np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))


def sigmoid(s):
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, np.ones_like(e), e) / (1 + e)


def fwd_bwd_ref(inn, out, c, o, neg, valid, reg, dtype):
    """dict of loss_t [B], s [B, 1 + K], centre / positive [B, D], noise [K, B, D] (k-major, as the kernel lays them out) and
    grads [(2 + K) B, D] in `dtype`, in the kernel's order: positive, then k ascending.  Ids outside the tables and
    valid == 0 give zeros; `bad` says whether any id lay outside."""
    V, W = np.asarray(inn).astype(dtype), np.asarray(out).astype(dtype)
    c, o, neg = np.asarray(c, np.int64), np.asarray(o, np.int64), np.asarray(neg, np.int64)
    B, K, ni = c.size, neg.shape[1], V.shape[0]
    inside = lambda a: (a >= 0) & (a < ni)                                      # noqa: E731
    bad = ~(inside(c) & inside(o) & inside(neg).all(1))
    ok = ~bad & (np.ones(B, bool) if valid is None else np.asarray(valid) != 0)
    c, o, neg = np.where(ok, c, 0), np.where(ok, o, 0), np.where(ok[:, None], neg, 0)
    v, wo = V[c], W[o]
    reg = dtype(reg)
    so = np.sum(v * wo, axis=1, dtype=dtype)
    loss = softplus(-so)
    ao = -sigmoid(-so)
    gc = ao[:, None] * wo
    positive = ao[:, None] * v + reg * wo
    s, noise = [so], []
    for k in range(K):
        wk = W[neg[:, k]]
        sk = np.sum(v * wk, axis=1, dtype=dtype)
        m = neg[:, k] != o
        ak = sigmoid(sk)
        loss = loss + np.where(m, softplus(sk), dtype(0))
        gc = np.where(m[:, None], gc + ak[:, None] * wk, gc)
        noise.append(np.where(m[:, None], ak[:, None] * v + reg * wk, dtype(0)))
        s.append(sk)
    gc = gc + reg * v
    keep = ok.astype(dtype)
    r = {"loss_t": (loss * keep).astype(dtype), "s": (np.stack(s, 1) * keep[:, None]).astype(dtype),
         "centre": (gc * keep[:, None]).astype(dtype), "positive": (positive * keep[:, None]).astype(dtype),
         "noise": (np.stack(noise) * keep[None, :, None]).astype(dtype), "bad": bool(bad.any())}
    r["grads"] = np.concatenate([r["centre"], r["positive"], r["noise"].reshape(K * B, -1)])
    return r


def objective(inn, out, c, o, neg, reg):
    """the fp64 loss of the slots as the issue states it, L2 term included (what the gradient rows differentiate)"""
    V, W = np.asarray(inn, np.float64), np.asarray(out, np.float64)
    v, wo = V[c], W[o]
    total = softplus(-(v * wo).sum(1)) + 0.5 * reg * ((v * v).sum(1) + (wo * wo).sum(1))
    for k in range(neg.shape[1]):
        wk = W[neg[:, k]]
        total = total + (neg[:, k] != o) * (softplus((v * wk).sum(1)) + 0.5 * reg * (wk * wk).sum(1))
    return float(total.sum())


def step_ref(tables, accums, c, o, neg, valid, reg, lr, optimizer, dtype, eps=EPS):
    """One whole step in `dtype` on (in, out) and their accumulators: a dict with fwd_bwd_ref's entries, loss (the mean over
    the valid slots) and "in", "out", "in_acc", "out_acc" after the update (oracle.optim's row-sparse Adagrad, or the same
    segment sums applied as SGD).  The out table's id list is [o ; neg[:, 0] ; .. ; neg[:, K - 1]], the engine's order."""
    r = fwd_bwd_ref(tables[0], tables[1], c, o, neg, valid, reg, dtype)
    B = len(c)
    n_valid = B if valid is None else int((np.asarray(valid) != 0).sum())
    r["loss"] = float(np.sum(r["loss_t"], dtype=np.float64)) / n_valid if n_valid else float("nan")
    parts = ((np.asarray(c, np.int64), r["grads"][:B]),
             (np.concatenate([np.asarray(o, np.int64), np.asarray(neg, np.int64).T.reshape(-1)]), r["grads"][B:]))
    for name, T, Ta, (ids, rows) in zip(("in", "out"), tables, accums, parts):
        T, Ta = np.asarray(T).astype(dtype), np.asarray(Ta).astype(dtype)
        if optimizer == "adagrad":
            T, Ta = o_optim.sparse_adagrad_update(T, Ta, ids, rows, lr, eps, dtype=dtype)
        else:
            T = T.copy()
            uniq, summed = o_optim.segment_sum_rows(ids, rows, dtype)
            T[uniq] = T[uniq] - dtype(lr) * summed
        r[name], r[name + "_acc"] = T, Ta
    return r


# ---- the planted corpus of the learning tests -------------------------------------------------------------------------------
PLANTED = dict(nd=200, ni=64, length=12, rank=8, batch=256, steps=400, window=3, negatives=5, seed=3, k=5)
CHANCE = 31.0 / 63.0


def planted_documents():
    """(indices int64, doc_offsets int64): 200 documents of 12 items over 64 items in two communities, each document drawn
    uniformly from one of them (the corpus of _bpr_ref.PLANTED as sequences)"""
    rng = np.random.default_rng(0)
    nd, ni, length = PLANTED["nd"], PLANTED["ni"], PLANTED["length"]
    docs = np.stack([rng.integers(0, ni // 2, length) + (ni // 2) * (d % 2) for d in range(nd)])
    return docs.reshape(-1).astype(np.int64), np.arange(nd + 1, dtype=np.int64) * length


def own_share(rows, k=PLANTED["k"]):
    """the share of each item's k nearest items by cosine (score descending, id ascending, itself left out) that come from
    its own community"""
    rows = np.asarray(rows, np.float64)
    unit = rows / np.maximum(np.sqrt((rows * rows).sum(1, keepdims=True)), 1e-300)
    sim = unit @ unit.T
    np.fill_diagonal(sim, -np.inf)
    top = np.argsort(-sim, axis=1, kind="stable")[:, :k]
    half = rows.shape[0] // 2
    return float(((top >= half) == (np.arange(rows.shape[0]) >= half)[:, None]).mean())


def planted_run(dtype=np.float64, optimizer="adagrad"):
    """(own-community share of the in rows' 5 nearest, every step's mean loss) of the reference loop on the planted corpus"""
    P = PLANTED
    indices, offsets = planted_documents()
    docs = [indices[offsets[d]:offsets[d + 1]].tolist() for d in range(P["nd"])]
    so, su, si = doc_csr(docs)
    keep, alias = alias_table(noise_masses(np.bincount(indices, minlength=P["ni"])))
    rng = np.random.default_rng(1)
    tables = [rng.standard_normal((P["ni"], P["rank"])) * P["rank"] ** -0.5 for _ in range(2)]
    accums = [np.full_like(t, ACC0) for t in tables]
    losses = []
    for k0 in range(0, P["steps"], 50):
        c, _, o, valid, neg, _ = sample_ref(so, su, si, P["nd"], P["ni"], P["window"], P["negatives"], keep, alias, P["seed"],
                                            k0, 50, P["batch"])
        for k in range(50):
            r = step_ref(tables, accums, c[k], o[k], neg[k], valid[k], 0.0, LR, optimizer, dtype)
            tables, accums = [r["in"], r["out"]], [r["in_acc"], r["out_acc"]]
            losses.append(r["loss"])
    return own_share(tables[0]), losses

"""Plain NumPy restatement of the rule of esr_rerank_rule.h: Maximal Marginal Relevance over a candidate list and intra-list
similarity.  No GPU, no torch: tests/test_rerank_ref.py checks it on the CPU, tests/test_gpu_rerank.py runs the kernels
against it.

Two flavours, chosen by `dtype`:
    np.float64   every product and sum in fp64 (oml = 1.0f - lam is still formed in float32: it is an input of the rule);
    np.float32   the chain the kernels run: per lane  acc = float32(float64(a) * float64(b) + float64(acc))  over the
                 lane's four elements from 0, the butterfly over the G lanes in float32, the penalty float32(oml * p) and
                 v = float32(float64(lam) * float64(rel) - float64(pen)).
Both flavours keep the summation ORDER of the rule (lane chains, then strides 1, 2, .. G / 2).  On exact tables (entries and
rel multiples of 2^-6 of magnitude <= 2, lam a multiple of 1/4) nothing rounds in either flavour, so any order gives the same
number and a caller may hand in the similarities as ``gram`` (rows @ rows.T in fp64): test_rerank_ref.py shows the equality.

On random tables the bound of tests/_bpr_ref.py holds:  kernel error against fp64 <= FACTOR * e32 + FLOOR * max(1, scale),
e32 the float32 flavour's own error against fp64.
"""
import numpy as np

FACTOR, FLOOR = 4.0, 2.0 ** -22
FAIL_POS, FAIL_REL = 1 << 30, 1 << 29
STAGE_BYTES, MAX_WIDTH = 128 * 1024, 1024


def lanes(D):
    G = 1
    while G < D // 4:
        G <<= 1
    return G


def staged(width, D):
    return width * D * 4 <= STAGE_BYTES


def sim_rows(A, b, dtype):
    """sim of every row of A [n, D] with b ([D] or [n, D]) in the rule's order, in `dtype`."""
    A = np.asarray(A, np.float32)
    b = np.broadcast_to(np.asarray(b, np.float32), A.shape)
    n, D = A.shape
    G = lanes(D)
    a4 = np.zeros((n, 4 * G), np.float64)
    b4 = np.zeros((n, 4 * G), np.float64)
    a4[:, :D], b4[:, :D] = A, b
    a4, b4 = a4.reshape(n, G, 4), b4.reshape(n, G, 4)
    acc = np.zeros((n, G), dtype)
    for e in range(4):
        acc = (a4[:, :, e] * b4[:, :, e] + acc.astype(np.float64)).astype(dtype)
    idx, stride = np.arange(G), 1
    while stride < G:
        acc = acc + acc[:, idx ^ stride]          # (an IEEE addition in `dtype`)
        stride <<= 1
    return acc[:, 0]


def value(lam, rel, p, dtype):
    """v = fmaf(lam, rel, -(oml * p)) on arrays"""
    lam32 = np.float32(lam)
    oml = np.float64(np.float32(1.0) - lam32)
    with np.errstate(invalid="ignore", over="ignore"):
        pen = (oml * np.asarray(p, np.float64)).astype(dtype)
        return (np.float64(lam32) * np.asarray(rel, np.float64) - pen.astype(np.float64)).astype(dtype)


def _present(rows, cand, rel, L):
    ni, width = rows.shape[0], cand.size
    inside = np.arange(width) < max(0, min(int(L), width))
    pos_bad = (cand < 0) | (cand >= ni)
    rel_bad = np.zeros(width, bool) if rel is None else ~np.isfinite(rel)
    failed = (FAIL_POS if (inside & pos_bad).any() else 0) | (FAIL_REL if (inside & rel_bad).any() else 0)
    return inside & ~pos_bad & ~rel_bad, failed


def mmr_query(rows, cand, rel, L, lam, n_out, dtype, gram=None, picks=None):
    """One query by the rule.  A dict: pos, item (int32[n_out]), rel, value (`dtype`[n_out]), length, failed and values
    (per round the array v[c], -inf where c is absent or picked).  ``gram`` [width, width]: the similarities handed in.
    ``picks``: follow these picks and not the rule's own (to recompute a kernel's rounds from its own history)."""
    cand, rel = np.asarray(cand, np.int64), np.asarray(rel, np.float32)
    width = cand.size
    live, failed = _present(rows, cand, rel, L)
    R = rows[np.where(live, cand, 0)]
    out = dict(pos=np.full(n_out, -1, np.int32), item=np.full(n_out, -1, np.int32), rel=np.zeros(n_out, np.float32),
               value=np.zeros(n_out, dtype), length=0, failed=failed, values=[])
    m = np.zeros(width, dtype)
    for t in range(n_out):
        v = value(lam, rel, np.zeros(width, dtype) if t == 0 else m, dtype)
        vv = np.where(live & ~np.isnan(v), v, -np.inf)
        if picks is None:
            if not np.any(vv > -np.inf):
                break
            s = int(np.argmax(vv))                 # (the first maximum: ties go to the smallest c)
        else:
            if t >= len(picks):
                break
            s = int(picks[t])
        out["pos"][t], out["item"][t], out["rel"][t], out["value"][t] = s, cand[s], rel[s], v[s]
        out["values"].append(vv)
        out["length"] = t + 1
        live[s] = False
        sim = gram[s].astype(dtype) if gram is not None else sim_rows(R, R[s], dtype)
        m = sim if t == 0 else np.fmax(m, sim)
    return out


def mmr_ref(rows, cand, rel, lengths, lam, n_out, dtype, grams=None):
    """Every query: (pos, item int32[nq, n_out], rel float32, value `dtype` [nq, n_out], length int32[nq], failed)."""
    nq, width = cand.shape
    res = [mmr_query(rows, cand[q], rel[q], width if lengths is None else lengths[q], lam, n_out, dtype,
                     None if grams is None else grams[q]) for q in range(nq)]
    failed = 0
    for r in res:
        failed |= r["failed"]
    return (np.stack([r["pos"] for r in res]), np.stack([r["item"] for r in res]), np.stack([r["rel"] for r in res]),
            np.stack([r["value"] for r in res]), np.array([r["length"] for r in res], np.int32), failed)


def gram_of(rows, cand):
    """fp64 rows[cand] @ rows[cand].T of one query (positions outside the table read row 0: never used)"""
    ni = rows.shape[0]
    R = rows[np.where((cand >= 0) & (cand < ni), cand, 0)].astype(np.float64)
    return R @ R.T


def ils_query(rows, cand, L, ks, dtype, gram=None, reverse_j=False, reverse_i=False):
    """(ils float32[nk], valid int32[nk], failed) of one query.  reverse_j / reverse_i run the row chain / the prefix
    backwards: NOT the rule -- what the order witnesses tell apart."""
    cand = np.asarray(cand, np.int64)
    width = cand.size
    L = max(0, min(int(L), width))
    kmax = min(ks[-1], L)
    present, failed = _present(rows, cand[:kmax], None, kmax)
    R = rows[np.where(present, cand[:kmax], 0)]
    r = np.zeros(kmax, np.float64)
    for i in range(kmax):
        js = np.flatnonzero(present[:i])
        if not present[i] or js.size == 0:
            continue
        sims = (gram[i, js] if gram is not None else sim_rows(R[js], R[i], dtype)).astype(np.float64)
        r[i] = np.cumsum(sims[::-1] if reverse_j else sims)[-1]          # (cumsum adds one by one, in order)
    ils, valid = np.zeros(len(ks), np.float32), np.zeros(len(ks), np.int32)
    for j, k in enumerate(ks):
        top = min(k, L)
        n = int(present[:top].sum())
        if n < 2:
            continue
        part = r[:top][present[:top]]
        P = np.cumsum(part[::-1] if reverse_i else part)[-1]
        ils[j], valid[j] = np.float32(P / (n * (n - 1) / 2)), 1
    return ils, valid, failed


def ils_ref(rows, cand, lengths, ks, dtype, grams=None):
    nq, width = cand.shape
    res = [ils_query(rows, cand[q], width if lengths is None else lengths[q], ks, dtype, None if grams is None else grams[q])
           for q in range(nq)]
    failed = 0
    for r in res:
        failed |= r[2]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), failed


# ---- cases ---------------------------------------------------------------------------------------------------------------
def exact_table(rng, ni, D):
    """float32 [ni, D]: multiples of 2^-6 of magnitude <= 2"""
    return (rng.integers(-128, 129, (ni, D)).astype(np.float32) / np.float32(64.0)).astype(np.float32)


def exact_rel(rng, shape):
    return (rng.integers(-128, 129, shape).astype(np.float32) / np.float32(64.0)).astype(np.float32)


def is_f32(x):
    """every entry of the fp64 array is a float32 number"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(x.astype(np.float32).astype(np.float64), x))


# the fp64 order witnesses of the intra-list similarity, rows of powers of two with D = 4
WITNESS_ROW_CHAIN = np.array([[1, 0, 0, 0], [0, 2.0 ** 26, 0, 0], [0, 0, -2.0 ** 26, 0], [1, 2.0 ** 27, 2.0 ** 27, 0]],
                             np.float32)
"""the last row's chain over j = 0, 1, 2 is 1 + 2^53 - 2^53: 0 in ascending j, 1 backwards; every other sim is 0"""
WITNESS_PREFIX = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 2.0 ** 26, 0, 0], [0, 2.0 ** 27, 0, 0], [0, 0, 2.0 ** 26, 0],
                           [0, 0, -2.0 ** 27, 0]], np.float32)
"""row sums r = 0, 1, 0, 2^53, 0, -2^53: the prefix is 0 in ascending i, 1 backwards"""

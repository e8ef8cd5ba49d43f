"""CPU oracle of ``factorization._recommend_rows`` for tests/test_gpu_recommend_cut.py, pinned by test_recommend_ref.py.

The scores are ``_als_ref.predict``'s (fp64 sum in ascending dimension, rounded once to float32) and the lists come from a
FULL sort by (score descending, item id ascending): no candidate stage, no cut.  ``score_table`` scores every (row, item)
once; ``full_order`` sorts every row once; ``lists`` cuts the lists of any k, any query order and any seen sets out of
those two, so one table serves every (k, slack, exclusion) case of a shape.  ``_als_ref.recommend`` is the same statement
per query and per call; test_recommend_ref.py holds the two against each other.

The candidate condition (``band_counts``).  On real-valued tables ``retrieve_topk(mode="exact")`` ranks by an f32
accumulation of the 9 bf16 plane products per dimension, while the final order is by the fp64 sum.  With

    tau_q = 2 * 9 D * 2^-24 * max_i sum_d |x_qd * y_id|        (twice the f32 accumulation error over 9 D products)

an item can stand before a listed item w in retrieval's order only if its fp64 score is at least ``s_w - tau_q``.  Those
are: the other k - 1 listed items, at most r_u <= r_max seen items, and the items that are neither listed nor above the
band -- the *band* ``[s_k - tau_q, s_k]`` below the k-th listed score s_k.  So with ``k' = k + r_max + slack`` candidates
every listed item is a candidate whenever the band holds at most ``slack`` items, and the list is then the full sort's.
Two details make the count here no smaller than that of the half-open band ``[s_k - tau_q, s_k)`` over fp64 scores: the
count runs over the float32-ROUNDED scores the lists are ordered by, the band widened by two float32 ulps of s_k for that
rounding, and it includes items that tie s_k without being listed (a higher id).  Seen items inside the band are counted
too (they are also within r_u: counted twice, never missed)."""
import numpy as np

import _als_ref as ref

F32, F64 = np.float32, np.float64


def grid(rng, shape, levels=8, step=4.0):
    """Values ``n / step`` with n in [-levels, levels]: multiples of 1/4 in [-2, 2] by default (test_gpu_retrieve._grid).
    Exact in bf16; every product and every sum of up to 128 of them is exact in f32 and in fp64."""
    return (rng.integers(-levels, levels + 1, shape) / step).astype(F32)


def is_grid(a, step=4.0, top=2.0):
    a = np.asarray(a, F64)
    return bool(np.all(a * step == np.round(a * step)) and np.all(np.abs(a) <= top))


def score_table(X, Y, offset=None):
    """float32[nu, ni]: ``_als_ref.predict`` of every (row of X, row of Y)."""
    nu, ni = X.shape[0], Y.shape[0]
    out = np.empty((nu, ni), F32)
    ipos = np.arange(ni)
    for u in range(nu):
        out[u] = ref.predict(X, Y, np.full(ni, u), ipos, offset)
    return out


def full_order(table, items):
    """int64[nu, ni]: per row the item positions by (score descending, item id ascending)."""
    items = np.asarray(items)
    return np.stack([np.lexsort((items, -row.astype(F64))) for row in table])


def lists(table, order, items, upos, seen, k):
    """(ids int32[nq, k] padded with -1, scores float32[nq, k] padded with 0, lengths int32[nq], places): query q is row
    ``upos[q]`` of the table (-1: unknown, an empty list); ``seen`` is None or a list with one array of item positions per
    ROW of the table, which are left out.  ``places[q]``: the listed items' places in the row's order WITHOUT exclusion."""
    items = np.asarray(items)
    nq, ni = len(upos), len(items)
    ids, scores, lengths, places = np.full((nq, k), -1, np.int32), np.zeros((nq, k), F32), np.zeros(nq, np.int32), []
    for q, u in enumerate(upos):
        if u < 0:
            places.append(np.zeros(0, np.int64))
            continue
        keep = np.ones(ni, bool)
        if seen is not None:
            keep[np.asarray(seen[u], np.int64)] = False
        at = np.flatnonzero(keep[order[u]])[:k]
        pos = order[u][at]
        ids[q, :len(pos)], scores[q, :len(pos)], lengths[q] = items[pos], table[u, pos], len(pos)
        places.append(at)
    return ids, scores, lengths, places


def tau(X, Y, upos):
    """float64[nq]: tau_q of the module text (0 for an unknown query)."""
    D = X.shape[1]
    absY = np.abs(Y.astype(F64))
    out = np.zeros(len(upos), F64)
    for q, u in enumerate(upos):
        if u >= 0:
            out[q] = 2.0 * 9 * D * 2.0 ** -24 * float((absY @ np.abs(X[u].astype(F64))).max())
    return out


def band_counts(table, ids, scores, lengths, items, upos, taus):
    """int64[nq]: per query the items that are not listed and whose float32 score lies in ``[s_k - tau_q - 2 ulp(s_k),
    s_k]``, s_k the last listed score -- the band count of the module text.  0 for an empty list."""
    items = np.asarray(items)
    out = np.zeros(len(upos), np.int64)
    for q, u in enumerate(upos):
        n = int(lengths[q])
        if u < 0 or n == 0:
            continue
        s_k = F64(scores[q, n - 1])
        low = s_k - taus[q] - 2.0 ** -22 * abs(s_k)
        row = table[u].astype(F64)
        listed = np.isin(items, ids[q, :n])
        out[q] = int(np.count_nonzero((row >= low) & (row <= s_k) & ~listed))
    return out


def qualifies(table, ids, scores, lengths, items, upos, taus, slack):
    """bool[nq]: the candidate condition -- the band holds at most ``slack`` items."""
    return band_counts(table, ids, scores, lengths, items, upos, taus) <= slack

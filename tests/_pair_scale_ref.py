"""NumPy-vectorised oracles of the pair-table family, for inputs above one launch grid (test_gpu_pair_scale.py).

The committed restatements (_cooccur_ref, _dice_ref, _terms_ref, _neighbours_ref) are Python loops over dictionaries: right
to read, hours to run on a million tokens.  Every function here states the SAME arithmetic over whole arrays -- integer
sums, one rounding to float32 where the restatement has one -- and test_pair_scale_ref.py holds each against its
restatement array for array and bit for bit, on the small fixtures of the host tests and on fresh random cases.  The GPU
tests compare only against these; that CPU test is what makes it legitimate.

Inputs are CSR: ``tokens`` (any integer array of ids in [0, 2^31 - 1]) with ``offsets int64[ndocs + 1]``; `unpack` gives
the list of documents back for the restatements.

GRID_ELEMS / GRID_WAVES restate the launch rule of esr_common.h (kBlock = 256 threads, kMaxGrid = 256 * 8 workgroups):
above GRID_ELEMS elements a one-thread-per-element kernel goes round its grid-stride loop, above GRID_WAVES items a
one-wave-per-item kernel does.  test_pair_scale_ref.py pins them against the header's text."""
import math

import numpy as np

from _cooccur_ref import lcm_upto
from _neighbours_ref import ref_scores

GRID_BLOCKS = 2048                    # kMaxGrid
GRID_ELEMS = GRID_BLOCKS * 256        # kMaxGrid * kBlock
GRID_WAVES = GRID_BLOCKS * 4          # kMaxGrid * (kBlock / kWave)


def unpack(tokens, offsets):
    return [tokens[offsets[d]:offsets[d + 1]] for d in range(len(offsets) - 1)]


def doc_of_position(offsets):
    """int64[N]: the document of every position (empty documents own none)."""
    offsets = np.asarray(offsets, np.int64)
    return np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))


def _sum_by_key(keys, weights):
    """(distinct keys ascending, exact int64 sums of their weights)."""
    order = np.argsort(keys, kind="stable")
    keys, weights = keys[order], weights[order]
    if keys.size == 0:
        return keys, weights
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[first], np.add.reduceat(weights, first)


# ---- window pairs (_cooccur_ref.ref_exact) ----
def vec_cooccur(tokens, offsets, W):
    """(index int64, other int64, count float32) ascending by (index, other).  _cooccur_ref's rule per unordered position
    pair (p, q = p + d) of one document: the key is (larger id, smaller id); equal ids never pair; the LATER token larger
    counts for d <= W, the EARLIER one larger only for d < W (the window reaches W back and W - 1 forward).  Weights are the
    integers lcm(1..W) // d, summed exactly in int64; count = float32(float64(sum) / float64(lcm))."""
    t = np.asarray(tokens, np.int64)
    start = np.asarray(offsets, np.int64)[doc_of_position(offsets)]
    L = lcm_upto(W)
    pos = np.arange(t.size, dtype=np.int64)
    keys, weights = [], []
    for d in range(1, W + 1):
        q = pos[pos - d >= start]
        tq, tp = t[q], t[q - d]
        live = (tq != tp) & ((tq > tp) | (d < W))
        tq, tp = tq[live], tp[live]
        keys.append((np.maximum(tq, tp) << 32) | np.minimum(tq, tp))
        weights.append(np.full(tq.size, L // d, np.int64))
    keys, sums = _sum_by_key(np.concatenate(keys), np.concatenate(weights))
    count = (sums.astype(np.float64) / np.float64(L)).astype(np.float32)
    return keys >> 32, keys & 0xFFFFFFFF, count


# ---- set pairs and document frequency (_dice_ref.ref_dice) ----
def vec_dice(tokens, offsets):
    """(index, other, count float32, ids, df float32) as ref_dice: per document the sorted distinct ids (one np.unique over
    document << 32 | id does every document at once), every i < j of them by np.triu_indices (documents with the same
    number of distinct ids share one call), then one np.unique(..., return_counts=True) over all keys."""
    t = np.asarray(tokens, np.int64)
    per_doc = np.unique((doc_of_position(offsets) << 32) | t)            # ascending by (document, id): the sorted sets
    doc, ident = per_doc >> 32, per_doc & 0xFFFFFFFF
    ids, df = np.unique(ident, return_counts=True)
    first = np.flatnonzero(np.concatenate([[True], doc[1:] != doc[:-1]])) if doc.size else np.zeros(0, np.int64)
    size = np.diff(np.concatenate([first, [doc.size]]))
    keys = []
    for u in np.unique(size):
        if u < 2:
            continue
        rows = ident[first[size == u][:, None] + np.arange(u)]            # [documents of u distinct ids, u]
        i, j = np.triu_indices(int(u), 1)
        keys.append(((rows[:, i] << 32) | rows[:, j]).reshape(-1))
    keys, count = np.unique(np.concatenate(keys) if keys else np.zeros(0, np.int64), return_counts=True)
    return keys >> 32, keys & 0xFFFFFFFF, count.astype(np.float32), ids, df.astype(np.float32)


# ---- term statistics, dictionary, lookups, tf-idf rows (_terms_ref) ----
def vec_stats(tokens, offsets):
    """(ids, frequency, doc_frequency) int64 ascending by id, as ref_stats."""
    t = np.asarray(tokens, np.int64)
    ids, frequency = np.unique(t, return_counts=True)
    in_docs = np.unique((doc_of_position(offsets) << 32) | t) & 0xFFFFFFFF
    df_ids, doc_frequency = np.unique(in_docs, return_counts=True)
    assert np.array_equal(ids, df_ids)
    return ids, frequency.astype(np.int64), doc_frequency.astype(np.int64)


def vec_dictionary(ids, frequency, doc_frequency, min_frequency=20, max_size=500000):
    """(ids, frequency, doc_frequency) int64 in index order, as ref_dictionary: frequency >= min, frequency descending,
    ties by ascending id, the first min(max_size, count)."""
    ids, frequency, doc_frequency = (np.asarray(x, np.int64) for x in (ids, frequency, doc_frequency))
    keep = frequency >= min_frequency
    ids, frequency, doc_frequency = ids[keep], frequency[keep], doc_frequency[keep]
    order = np.lexsort((ids, -frequency))[:max(0, min(int(max_size), ids.size))]
    return ids[order], frequency[order], doc_frequency[order]


def _index_of(tokens, dict_ids):
    """int64[N]: the dictionary index of every token, -1 outside (dict_ids distinct)."""
    t, dict_ids = np.asarray(tokens, np.int64), np.asarray(dict_ids, np.int64)
    if dict_ids.size == 0:
        return np.full(t.size, -1, np.int64)
    order = np.argsort(dict_ids, kind="stable")
    at = np.minimum(np.searchsorted(dict_ids[order], t), dict_ids.size - 1)
    return np.where(dict_ids[order][at] == t, order[at], -1).astype(np.int64)


def vec_embedding(tokens, dict_ids, buckets=None):
    """(index_of int64[N] with -1 outside, embedding_index int64[N]), as ref_embedding."""
    t = np.asarray(tokens, np.int64)
    index = _index_of(t, dict_ids)
    bucket = np.asarray(buckets, np.int64) if buckets is not None else t & 0xFFFF
    return index, np.where(index >= 0, 1 + index, 1 + len(dict_ids) + bucket).astype(np.int64)


def wave_norm(squares, starts, lengths):
    """float64 per row: the sum of squares[starts[r] : starts[r] + lengths[r]] in the order of terms_tfidf_rows_kernel --
    lane l of 64 adds the entries l, l + 64, l + 128, ... of the row one by one, then six butterfly steps
    v += v[lane ^ s], s = 1, 2, 4, 8, 16, 32 (an fp64 add commutes, so every lane ends on the same bits)."""
    lanes = np.zeros((len(starts), 64), np.float64)
    lane = np.arange(64)
    for j in range(0, int(lengths.max()) if len(lengths) else 0, 64):
        live = (j + lane)[None, :] < lengths[:, None]
        at = np.where(live, starts[:, None] + j + lane[None, :], 0)
        lanes = lanes + np.where(live, squares[at] if squares.size else 0.0, 0.0)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, lane ^ s]
    return lanes[:, 0]


def _sequential_norm(squares, starts, lengths):
    """float64 per row: squares[starts[r]], then + the next, and so on -- rows advance together, one entry per step."""
    norm = np.zeros(len(starts), np.float64)
    for j in range(int(lengths.max()) if len(lengths) else 0):
        live = np.flatnonzero(lengths > j)
        norm[live] = norm[live] + squares[starts[live] + j]
    return norm


def vec_sparse_docs(tokens, offsets, dict_ids, doc_frequency, max_doc_frequency, stopwords=(), order="insertion"):
    """(out_offsets int64[ndocs + 1], token_index int64[nnz], token_tfidf float32[nnz]) as ref_sparse_docs: stopwords (raw
    ids) skipped, tokens outside the dictionary dropped, tf counts every occurrence; in fp64 idf = max(0, log1p(max_df) -
    log1p(df) + 1) with math.log1p, tfidf = tf * idf, norm = the sum of tfidf^2, value = float32(tfidf * (1 / sqrt(norm)))
    or 0 where norm == 0; rows ascending by index.  `order` is the order of the norm's sum: "insertion" (first occurrence:
    ref_sparse_docs), "ascending" (by index: ref_sparse_docs(ascending=True)) or "wave" (wave_norm: the kernel's)."""
    t = np.asarray(tokens, np.int64)
    ndocs = len(offsets) - 1
    index = _index_of(t, dict_ids)
    if len(stopwords):
        index[np.isin(t, np.array(sorted(int(s) for s in stopwords), np.int64))] = -1
    kept = np.flatnonzero(index >= 0)
    key, first_pos, tf = np.unique((doc_of_position(offsets)[kept] << 32) | index[kept], return_index=True,
                                   return_counts=True)
    doc, index = key >> 32, key & 0xFFFFFFFF
    df = np.asarray(doc_frequency, np.int64)[index]
    log_max_num_docs = math.log1p(max_doc_frequency)
    distinct_df, which = np.unique(df, return_inverse=True)
    idf = np.array([max(0.0, log_max_num_docs - math.log1p(int(d)) + 1.0) for d in distinct_df], np.float64)[which]
    tfidf = tf.astype(np.float64) * idf.reshape(-1)
    out_offsets = np.concatenate([[0], np.cumsum(np.bincount(doc, minlength=ndocs))]).astype(np.int64)
    starts, lengths = out_offsets[:-1], np.diff(out_offsets)
    squares = tfidf * tfidf
    if order == "wave":
        norm = wave_norm(squares, starts, lengths)
    elif order == "ascending":
        norm = _sequential_norm(squares, starts, lengths)
    else:
        assert order == "insertion"
        norm = _sequential_norm(squares[np.lexsort((first_pos, doc))], starts, lengths)
    inorm = np.zeros(ndocs, np.float64)
    inorm[norm > 0.0] = 1.0 / np.sqrt(norm[norm > 0.0])
    return out_offsets, index, (tfidf * inorm[doc]).astype(np.float32)


# ---- neighbours (_neighbours_ref.ref_neighbours) ----
def vec_neighbours(index, other, count, ids, df, k, orientation="both", score="dice"):
    """(ids int32[u], neighbours int32[u, k] padded -1, scores / counts float32[u, k] padded 0, lengths int32[u]) as
    ref_neighbours: the entry list of "stored" or -- every entry followed by its mirror -- "both", the f32 score of
    ref_scores, np.lexsort by (row, score descending, partner ascending), the first k of every row."""
    index, other = np.asarray(index, np.int64), np.asarray(other, np.int64)
    if ids is None:
        ids = np.unique(np.concatenate([index, other]))
    ids = np.asarray(ids, np.int64)
    u = ids.size
    s = ref_scores(index, other, count, ids, df, score) if u else np.zeros(0, np.float32)
    count = np.asarray(count, np.float32)
    row, partner = index, other
    if orientation == "both":
        row, partner = np.stack([index, other], 1).reshape(-1), np.stack([other, index], 1).reshape(-1)
        s, count = np.repeat(s, 2), np.repeat(count, 2)
    at = np.searchsorted(ids, row)
    for x in (index, other):
        where = np.minimum(np.searchsorted(ids, x), max(u - 1, 0))
        if x.size and (u == 0 or not np.array_equal(ids[where], x)):
            raise KeyError(int(x[0] if u == 0 else x[ids[where] != x][0]))
    order = np.lexsort((partner, -s.astype(np.float64), at))
    at, partner, s, count = at[order], partner[order], s[order], count[order]
    sizes = np.bincount(at, minlength=u)
    rank = np.arange(at.size) - (np.cumsum(sizes) - sizes)[at]
    keep = rank < k
    nb = np.full((u, k), -1, np.int32)
    sc = np.zeros((u, k), np.float32)
    ct = np.zeros((u, k), np.float32)
    nb[at[keep], rank[keep]] = partner[keep]
    sc[at[keep], rank[keep]] = s[keep]
    ct[at[keep], rank[keep]] = count[keep]
    return ids.astype(np.int32), nb, sc, ct, np.minimum(sizes, k).astype(np.int32)

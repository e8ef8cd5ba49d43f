"""CPU restatement of esrecsys_amd/wikipedia/neighbours.py, pure NumPy and Python: dict-of-lists rows, ``sorted`` with
the key ``(-score, id)``, sequential ``np.float32`` sums in history position order.  The oracle of the GPU tests; pinned
itself on a hand-worked table by test_neighbours_ref.py."""
import numpy as np


def ref_scores(index, other, count, ids, df, score):
    """float32 per entry: the joint count, or count / (df[other] + df[index]) in f32 (one add, one division)."""
    count = np.asarray(count, np.float32)
    if score == "count":
        return count.copy()
    ids = np.asarray(ids, np.int64)
    df = np.asarray(df, np.float32)
    pi = np.searchsorted(ids, np.asarray(index, np.int64))
    po = np.searchsorted(ids, np.asarray(other, np.int64))
    return (count / (df[po] + df[pi])).astype(np.float32)


def ref_neighbours(index, other, count, ids, df, k, orientation="both", score="dice"):
    """(ids int32[u], neighbours int32[u, k] padded -1, scores / counts float32[u, k] padded 0, lengths int32[u])."""
    index, other = np.asarray(index, np.int64), np.asarray(other, np.int64)
    if ids is None:
        ids = np.unique(np.concatenate([index, other]))
    ids = np.asarray(ids, np.int64)
    known = set(ids.tolist())
    for x in np.concatenate([index, other]).tolist():
        if x not in known:
            raise KeyError(x)
    s = ref_scores(index, other, count, ids, df, score)
    count = np.asarray(count, np.float32)
    rows = {}
    for e in range(index.size):
        a, b = int(index[e]), int(other[e])
        rows.setdefault(a, []).append((s[e], b, count[e]))
        if orientation == "both":
            rows.setdefault(b, []).append((s[e], a, count[e]))
    u = ids.size
    nb = np.full((u, k), -1, np.int32)
    sc = np.zeros((u, k), np.float32)
    ct = np.zeros((u, k), np.float32)
    lengths = np.zeros(u, np.int32)
    for r, x in enumerate(ids.tolist()):
        row = sorted(rows.get(x, []), key=lambda t: (-float(t[0]), t[1]))[:k]
        lengths[r] = len(row)
        for j, (sj, pj, cj) in enumerate(row):
            nb[r, j], sc[r, j], ct[r, j] = pj, sj, cj
    return ids.astype(np.int32), nb, sc, ct, lengths


def ref_candidate_sums(table, query, reverse=False):
    """{candidate: np.float32 sum} of one query (a list of ids): over the history positions in ascending order (or
    descending with `reverse`), each row's kept entries added one by one into an np.float32."""
    ids, nb, sc, _ct, lengths = table
    row_of = {int(x): r for r, x in enumerate(ids.tolist())}
    sums = {}
    positions = range(len(query) - 1, -1, -1) if reverse else range(len(query))
    for p in positions:
        r = row_of.get(int(query[p]))
        if r is None:
            continue
        for j in range(int(lengths[r])):
            c = int(nb[r, j])
            sums[c] = np.float32(sums[c] + sc[r, j]) if c in sums else np.float32(sc[r, j])
    return sums


def ref_recommend(table, history, offsets, k, exclude_history=True):
    """(rec_ids int32[nq, k] padded -1, rec_scores float32[nq, k] padded 0, rec_lengths int32[nq])."""
    history, offsets = np.asarray(history, np.int64), np.asarray(offsets, np.int64)
    nq = offsets.size - 1
    out_ids = np.full((nq, k), -1, np.int32)
    out_sc = np.zeros((nq, k), np.float32)
    out_len = np.zeros(nq, np.int32)
    for q in range(nq):
        query = history[offsets[q]:offsets[q + 1]].tolist()
        sums = ref_candidate_sums(table, query)
        if exclude_history:
            for h in query:
                sums.pop(int(h), None)
        best = sorted(sums.items(), key=lambda t: (-float(t[1]), t[0]))[:k]
        out_len[q] = len(best)
        for j, (c, v) in enumerate(best):
            out_ids[q, j], out_sc[q, j] = c, v
    return out_ids, out_sc, out_len

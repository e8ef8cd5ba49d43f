"""NumPy oracle of esrecsys_amd.evaluate: a plain loop per query, float64 in ascending rank order, the same two discount
tables the kernel reads (made here from their definition, not taken from the package), one rounding to float32."""
import numpy as np

F32 = np.float32


def tables(kmax, kideal):
    """disc[r - 1] = 1 / log2(r + 1) for r <= kmax; cum_disc = [0, cumsum(disc)] continued to kideal"""
    n = max(kmax, kideal)
    disc = 1.0 / np.log2(np.arange(2, n + 2, dtype=np.float64))
    cum = np.concatenate([np.zeros(1), np.cumsum(disc)])
    return disc[:kmax], cum[:kideal + 1]


def ranking_metrics(rec_ids, rec_lengths, truth, truth_offsets, ks, count_repeats=False, truth_size="distinct"):
    """dict of arrays shaped as RankingMetrics' tensors (ap / ndcg None with count_repeats)"""
    rec_ids, truth, off = np.asarray(rec_ids), np.asarray(truth), np.asarray(truth_offsets, dtype=np.int64)
    nq, width = rec_ids.shape
    nk = len(ks)
    kmax = min(ks[-1], width)
    longest = int(np.diff(off).max()) if nq else 0
    disc, cum = tables(kmax, min(ks[-1], longest))
    out = {"hits": np.zeros((nq, nk), np.int32), "first_hit": np.zeros(nq, np.int32), "valid": np.zeros(nq, np.int32)}
    for name in ("precision", "recall", "rr", "ap", "ndcg"):
        out[name] = np.zeros((nq, nk), F32)
    for q in range(nq):
        listed = truth[off[q]:off[q + 1]]
        wanted = set(listed.tolist())
        n_rel = len(listed) if truth_size == "listed" else len(wanted)
        if n_rel == 0:
            continue
        out["valid"][q] = 1
        length = width if rec_lengths is None else int(rec_lengths[q])
        seen = set()
        c, first, j = 0, 0, 0
        ap_sum, dcg = np.float64(0.0), np.float64(0.0)

        def emit(j):
            k = ks[j]
            m = min(k, n_rel)
            out["hits"][q, j] = c
            out["precision"][q, j] = F32(np.float64(c) / np.float64(k))
            out["recall"][q, j] = F32(np.float64(c) / np.float64(n_rel))
            out["rr"][q, j] = F32(np.float64(1.0) / np.float64(first)) if first else F32(0)
            out["ap"][q, j] = F32(ap_sum / np.float64(m))
            out["ndcg"][q, j] = F32(dcg / cum[m])

        for r in range(1, min(length, kmax) + 1):
            while j < nk and ks[j] < r:
                emit(j)
                j += 1
            v = int(rec_ids[q, r - 1])
            if v in wanted and (count_repeats or v not in seen):
                c += 1
                first = first or r
                ap_sum = ap_sum + np.float64(c) / np.float64(r)
                dcg = dcg + disc[r - 1]
            seen.add(v)
        while j < nk:
            emit(j)
            j += 1
        out["first_hit"][q] = first
    if count_repeats:
        out["ap"] = out["ndcg"] = None
    return out


def mean(metrics):
    """sequential float64 sums over the valid queries, in query order"""
    valid = np.flatnonzero(metrics["valid"])
    out = {"n_valid": int(valid.size)}
    for name in ("precision", "recall", "rr", "ap", "ndcg"):
        if metrics[name] is None:
            out[name] = None
            continue
        s = np.zeros(metrics[name].shape[1], np.float64)
        for q in valid:
            s = s + metrics[name][q].astype(np.float64)
        out[name] = s / valid.size if valid.size else s
    return out


def split_holdout(indices, doc_offsets, context=5, min_length=10, mode="first"):
    """make_training.py:74-98 at id level, as a loop over the documents"""
    indices, off = np.asarray(indices), np.asarray(doc_offsets, dtype=np.int64)
    ctx, tru, c_off, t_off, kept = [], [], [0], [0], []
    for d in range(off.size - 1):
        doc = [int(v) for v in indices[off[d]:off[d + 1]]]
        if len(doc) < min_length:
            continue
        kept.append(d)
        cut = context if mode == "first" else len(doc) - context
        ctx += doc[:cut]
        tru += doc[cut:]
        c_off.append(len(ctx))
        t_off.append(len(tru))
    return (np.array(ctx, np.int32), np.array(c_off, np.int64), np.array(tru, np.int32), np.array(t_off, np.int64),
            np.array(kept, np.int64))

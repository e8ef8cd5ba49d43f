"""CPU restatement of esrecsys_amd/ratings.py, pure NumPy and Python: dictionaries and loops, Python ints for the four
sums, ``np.float64`` scalars for every rounded operation.  The oracle of the GPU tests; pinned itself on a hand-worked
example by test_ratings_ref.py."""
import numpy as np


def ref_latest(user, item, rating, tstamp):
    """(user, item, rating) lists ascending by (user, item): the row with the largest tstamp, the later one on a tie."""
    best = {}
    for n, (u, i, r, t) in enumerate(zip(user, item, rating, tstamp)):
        key = (int(u), int(i))
        if key not in best or (t, n) >= best[key][:2]:
            best[key] = (t, n, r)
    keys = sorted(best)
    return [k[0] for k in keys], [k[1] for k in keys], [best[k][2] for k in keys]


def ref_deviations(user, rating, frac_bits=12):
    """(users ascending, mean float64 per user, dev Python ints per row): mean = the float64 sum in row order / count."""
    total, count = {}, {}
    for u, r in zip(user, rating):
        u = int(u)
        total[u] = np.float64(total.get(u, np.float64(0.0)) + np.float64(r))
        count[u] = count.get(u, 0) + 1
    users = sorted(total)
    mean = {u: np.float64(total[u] / np.float64(count[u])) for u in users}
    dev = [int(np.round((np.float64(r) - mean[int(u)]) * np.float64(2.0 ** frac_bits))) for u, r in zip(user, rating)]
    return users, [mean[u] for u in users], dev


def ref_sums(user, item, dev):
    """{(a, b): [n, P, Qa, Qb]} with a < b, Python ints: per item every pair of its raters."""
    by_item = {}
    for u, i, d in zip(user, item, dev):
        by_item.setdefault(int(i), []).append((int(u), int(d)))
    sums = {}
    for raters in by_item.values():
        raters.sort()
        for p in range(len(raters)):
            for q in range(p + 1, len(raters)):
                (a, da), (b, db) = raters[p], raters[q]
                assert a < b, "a (user, item) occurs twice"
                s = sums.setdefault((a, b), [0, 0, 0, 0])
                s[0] += 1
                s[1] += da * db
                s[2] += da * da
                s[3] += db * db
    return sums


def ref_sim(P, Qa, Qb):
    return np.float32(np.float64(P) / (np.sqrt(np.float64(Qa)) * np.sqrt(np.float64(Qb))))


def ref_similarity(sums, min_overlap=1, min_similarity=None):
    """(index int32, other int32, sim float32, overlap int32, dropped_flat) ascending by (index, other)."""
    index, other, sim, overlap, flat = [], [], [], [], 0
    for (a, b) in sorted(sums):
        n, P, Qa, Qb = sums[(a, b)]
        if Qa == 0 or Qb == 0:
            flat += 1
            continue
        s = ref_sim(P, Qa, Qb)
        if n < min_overlap or (min_similarity is not None and s <= np.float32(min_similarity)):
            continue
        index.append(a), other.append(b), sim.append(s), overlap.append(n)
    return (np.array(index, np.int32), np.array(other, np.int32), np.array(sim, np.float32), np.array(overlap, np.int32),
            flat)


def vec_similarity(user, item, dev, min_overlap=1, min_similarity=None):
    """``ref_similarity(ref_sums(user, item, dev), min_overlap, min_similarity)`` restated with arrays, for inputs of
    half a million pairs: per item the raters ascending and ``np.triu_indices`` over them, the pairs of all items reduced
    by their 64-bit key ``a << 32 | b`` in int64 (the sums stay below 2^53, the builder's own bound), and ``ref_sim``'s
    three roundings taken on whole arrays.  Pinned to the loop version, array for array, by test_ratings_ref.py."""
    user, item, dev = (np.asarray(x, np.int64) for x in (user, item, dev))
    order = np.lexsort((user, item))
    user, item, dev = user[order], item[order], dev[order]
    cut = np.flatnonzero(np.diff(item)) + 1
    key, P, Qa, Qb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [item.size]])):
        u, d = user[a:b], dev[a:b]
        assert (np.diff(u) > 0).all(), "a (user, item) occurs twice"
        p, q = np.triu_indices(u.size, 1)
        key.append((u[p] << 32) | u[q]), P.append(d[p] * d[q]), Qa.append(d[p] * d[p]), Qb.append(d[q] * d[q])
    key, P, Qa, Qb = (np.concatenate(x) for x in (key, P, Qa, Qb))
    if key.size == 0:
        return ref_similarity({}, min_overlap, min_similarity)
    keys, inverse, n = np.unique(key, return_inverse=True, return_counts=True)
    by_key = np.argsort(inverse, kind="stable")
    first = np.concatenate([[0], np.cumsum(n)[:-1]])
    P, Qa, Qb = (np.add.reduceat(x[by_key], first) for x in (P, Qa, Qb))
    flat = (Qa == 0) | (Qb == 0)
    with np.errstate(all="ignore"):
        sim = (P.astype(np.float64) / (np.sqrt(Qa.astype(np.float64)) * np.sqrt(Qb.astype(np.float64)))).astype(np.float32)
    keep = ~flat & (n >= min_overlap)
    if min_similarity is not None:
        keep &= ~(sim <= np.float32(min_similarity))
    return ((keys[keep] >> 32).astype(np.int32), (keys[keep] & 0xFFFFFFFF).astype(np.int32), sim[keep],
            n[keep].astype(np.int32), int(flat.sum()))


class RefUserKnn:
    """table = (ids, neighbours, scores, counts, lengths) as tests/_neighbours_ref.ref_neighbours returns it."""

    def __init__(self, table, user, item, rating, users, mean):
        self.ids, self.nb, self.sc, _ct, self.lengths = table
        self.row_of = {int(x): r for r, x in enumerate(np.asarray(self.ids).tolist())}
        self.mean = {int(u): np.float64(m) for u, m in zip(users, mean)}
        self.rated = {}
        for u, i, r in zip(user, item, rating):
            self.rated.setdefault(int(u), {})[int(i)] = np.float32(r)

    def affinity(self, A, i, center="neighbour", denominator="rated"):
        """(np.float32 affinity, support) -- (NaN, 0) for a user the table lacks."""
        A, i = int(A), int(i)
        if A not in self.row_of or A not in self.mean:
            return np.float32(np.nan), 0
        r = self.row_of[A]
        mean_a = self.mean[A]
        num, den, support = np.float64(0.0), np.float64(0.0), 0
        if denominator == "all":
            for j in range(int(self.lengths[r])):
                den = np.float64(den + np.float64(self.sc[r, j]))
        for j in range(int(self.lengths[r])):
            U = int(self.nb[r, j])
            if U not in self.mean or i not in self.rated.get(U, {}):
                continue
            s = np.float64(self.sc[r, j])
            c = mean_a if center == "query" else self.mean[U]
            num = np.float64(num + np.float64(s * np.float64(np.float64(self.rated[U][i]) - c)))
            if denominator == "rated":
                den = np.float64(den + abs(s))
            support += 1
        with np.errstate(all="ignore"):
            aff = np.float32(mean_a if support == 0 or den == 0 else np.float64(mean_a + np.float64(num / den)))
        return np.float32(aff + np.float32(0.0)), support          # -0 -> +0

    def predict(self, users, items, center="neighbour", denominator="rated"):
        out = [self.affinity(u, i, center, denominator) for u, i in zip(users, items)]
        return np.array([a for a, _ in out], np.float32), np.array([s for _, s in out], np.int32)

    def gathered(self, A):
        r = self.row_of.get(int(A))
        if r is None:
            return 0
        return sum(len(self.rated.get(int(self.nb[r, j]), {})) for j in range(int(self.lengths[r]))
                   if int(self.nb[r, j]) in self.mean)

    def recommend(self, users, k, exclude_rated=True, min_support=1, center="neighbour", denominator="rated"):
        nq = len(users)
        out_ids = np.full((nq, k), -1, np.int32)
        out_sc = np.zeros((nq, k), np.float32)
        out_len = np.zeros(nq, np.int32)
        for q, A in enumerate(users):
            A = int(A)
            if A not in self.row_of or A not in self.mean:
                continue
            r = self.row_of[A]
            cands = set()
            for j in range(int(self.lengths[r])):
                U = int(self.nb[r, j])
                if U in self.mean:
                    cands |= set(self.rated.get(U, {}))
            if exclude_rated:
                cands -= set(self.rated.get(A, {}))
            scored = []
            for i in cands:
                aff, support = self.affinity(A, i, center, denominator)
                if support >= min_support:
                    scored.append((aff, i))
            best = sorted(scored, key=lambda t: (-float(t[0]), t[1]))[:k]
            out_len[q] = len(best)
            for j, (aff, i) in enumerate(best):
                out_ids[q, j], out_sc[q, j] = i, aff
        return out_ids, out_sc, out_len

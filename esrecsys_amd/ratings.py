"""Explicit ratings: the Pearson user-similarity table and the user-kNN affinity over it, on the GPU (esr_ratings.hip) --
the collaborative-filtering job that the reference's book builds first (chapter 5, "Data Processing": the daily offline
job from ``(user, item, rating, timestamp)`` rows to ``USim`` and, as the exercise it leaves open, to ``Aff``).

    user, item, rating = latest_ratings(user, item, rating, tstamp)            # the most recent rating of a pair
    users, mean, dev = rating_deviations(user, rating, frac_bits=12)           # per-user mean, fixed-point deviations
    b = UserSimilarityBuilder().add(user, item, dev)                            # any number of item-disjoint adds
    index, other, sim, overlap = b.finalize(min_overlap=2)                      # index < other, ascending (index, other)
    table = neighbours(index, other, sim, users, None, k=5, orientation="both", score="count")
    model = UserKnn(table, user, item, rating, users, mean)
    aff, support = model.predict(query_users, query_items)
    rec_ids, rec_scores, rec_lengths = model.recommend(query_users, k=500)      # straight into evaluate.ranking_metrics

Similarity.  With d[u, i] = r[u, i] - mean[u] and I(a, b) the items both users rated,

    USim[a, b] = sum_I d[a, i] d[b, i] / (sqrt(sum_I d[a, i]^2) sqrt(sum_I d[b, i]^2))

The deviations are rounded once to fixed point, ``dev = int32(round_half_even(d * 2^frac_bits))``, and per user pair four
INTEGER sums are reduced in a hash table on the device: n (the overlap), P = sum dev_a dev_b, Qa = sum dev_a^2, Qb = sum
dev_b^2.  Integer sums do not depend on the order of the atomics, on how the items are cut into launches or on how they are
divided among ``add`` calls, and the scale 2^frac_bits cancels: ``sim = float32(float64(P) / (sqrt(float64(Qa)) *
sqrt(float64(Qb))))`` -- a NumPy restatement gives the same bits.  Exactness bound: with m = the largest |dev| and I = the
number of distinct items given so far, ``m^2 I < 2^53`` is checked before any launch, so every sum is an integer that a
double holds exactly.

Two stated deviations from the book.  (1) Its job yields a null similarity where a user's deviations over the common items
are all zero (0 / 0); here such an entry is dropped and counted in ``builder.dropped_flat``.  (2) Its listing divides by
``sqrt(sum_of_sqrd_devs_2)`` twice; this follows its equation (both users' sums) instead.

Affinity.  For the query user A, the item i and A's table row (neighbour U_j, similarity s_j, j ascending), the columns
counted are those whose U_j rated i; ``support`` is their number and

    num = sum s_j (float64(r[U_j, i]) - c_j)      c_j = mean[A]   (center="query", the book's printed form)
                                                  c_j = mean[U_j] (center="neighbour", Resnick's form: the default)
    den = sum |s_j| over the counted columns      (denominator="rated": the default)
    den = sum s_j over the whole row              (denominator="all", as printed)
    aff = float32(mean[A] + num / den)            and mean[A] when support == 0 or den == 0

in float64, in ascending column order, every operation rounded once (-0 is returned as +0).
"""
import numpy as np
import torch

from . import ops
from .wikipedia.neighbours import MAX_K
from .wikipedia.pair_table import FAILURES as TABLE_FAILURES, CooccurrenceError, PairTable, plan_ranges  # noqa: F401

FAILURES = dict(TABLE_FAILURES)
FAILURES[2] = "a negative id"
FAILURES[4] = "item offsets or a tile prefix that are not the host's plan"
FAILURES[128] = "a (user, item) given twice in one add (the users of an item are not strictly ascending)"
CENTERS = ("query", "neighbour")
DENOMINATORS = ("rated", "all")


def _tensor(x, what):
    if isinstance(x, torch.Tensor):
        return x.reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).reshape(-1)


def _same_length(what, *xs):
    if len({int(x.numel()) for x in xs}) != 1:
        raise ValueError("%s must have one length, got %s" % (what, [int(x.numel()) for x in xs]))


def latest_ratings(user, item, rating, tstamp):
    """The book's "most recent rating for a pair": of the rows that share (user, item) the one with the largest `tstamp`
    stays (of equal timestamps, the one given last).  Returns (user int32, item int32, rating) ascending by (user, item),
    on the inputs' device.  Two stable sorts and segment ends in torch: plumbing, not a hot path."""
    user, item, rating, tstamp = (_tensor(x, n) for x, n in ((user, "user"), (item, "item"), (rating, "rating"),
                                                             (tstamp, "tstamp")))
    _same_length("user, item, rating and tstamp", user, item, rating, tstamp)
    dev = user.device
    item, rating, tstamp = item.to(dev), rating.to(dev), tstamp.to(dev)
    key = (user.to(torch.int64) << 32) + item.to(torch.int64)
    by_time = torch.sort(tstamp, stable=True).indices
    by_key = torch.sort(key[by_time], stable=True)
    order = by_time[by_key.indices]
    k = by_key.values
    last = torch.ones(k.numel(), dtype=torch.bool, device=dev)
    if k.numel() > 1:
        last[:-1] = k[1:] != k[:-1]
    keep = order[last]
    return user[keep].to(torch.int32), item[keep].to(torch.int32), rating[keep]


def rating_deviations(user, rating, frac_bits=12):
    """(users int32[nu] ascending, mean float64[nu], dev int32[N]): the mean rating of every user and, per input row,
    ``dev = int32(round_half_even((rating - mean[user]) * 2^frac_bits))`` computed in float64.

    The mean is a float64 torch sum (``index_add_``) divided by the count.  On the device that sum is made of atomic adds,
    so it is independent of their order exactly when every partial sum is representable: ratings that are multiples of
    2^-k with ``sum |rating| < 2^(53 - k)`` per user (half-star ratings: k = 1) -- then the mean is the correctly rounded
    quotient of two exact numbers.  Other ratings give a mean that may differ in its last bit from run to run."""
    frac_bits = int(frac_bits)
    if not 0 <= frac_bits <= 30:
        raise ValueError("frac_bits = %d outside [0, 30]" % frac_bits)
    user, rating = _tensor(user, "user"), _tensor(rating, "rating")
    _same_length("user and rating", user, rating)
    rating = rating.to(device=user.device, dtype=torch.float64)
    users, inverse, counts = torch.unique(user.to(torch.int64), return_inverse=True, return_counts=True)
    total = torch.zeros(users.numel(), dtype=torch.float64, device=user.device).index_add_(0, inverse, rating)
    mean = total / counts.to(torch.float64)
    scaled = torch.round((rating - mean[inverse]) * float(1 << frac_bits))
    if scaled.numel() and float(scaled.abs().max()) >= 2.0 ** 31:
        raise ValueError("a deviation does not fit int32 at frac_bits = %d; lower frac_bits" % frac_bits)
    return users.to(torch.int32), mean, scaled.to(torch.int32)


class UserSimilarityBuilder:
    """Reduce-by-key of the co-rating user pairs in the WIDE pair table of esr_wide_table.h (open addressing, 64-bit keys
    ``index << 32 | other``, four uint64 sums per slot), modelled on ``DiceBuilder``.

    ``add`` sorts its rows by (item, user) (torch: plumbing) and hands the kernel CSR-by-item lists of (user, dev).  An
    item's raters must arrive in ONE ``add``: the builder keeps the item ids it has seen and refuses a repeated one with
    ``ValueError`` before any launch.  Growth rule (``PairTable``): an item of n raters emits n (n - 1) / 2 pairs; an
    ``add`` is cut into item ranges whose bound is at most ``max_pairs_per_launch`` (``plan_ranges``: an item is never
    cut) and the bound is reserved before each launch.  The kernel's work unit is a tile of one item's triangle; the
    prefix of the tile counts is made HERE from the item offsets the plan needs anyway.

    A failure word raised by the device -- a negative id, a (user, item) given twice -- becomes a ``CooccurrenceError`` and
    leaves the builder unusable, as in the other builders."""

    def __init__(self, capacity=1 << 20, device=None, max_pairs_per_launch=1 << 26):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_pairs_per_launch = max(int(max_pairs_per_launch), 1)
        self.launches = 0
        self.dropped_flat = 0
        self._max_user = -1
        self._max_dev = 0
        self._items = np.zeros(0, np.int64)     # the item ids seen so far, ascending
        self._pairs = PairTable(capacity, self.device, FAILURES, "user-similarity table",
                                table_ops=(ops.usersim_table, ops.usersim_rehash))

    capacity = property(lambda self: self._pairs.capacity)
    rehashes = property(lambda self: self._pairs.rehashes)

    @staticmethod
    def tiles_of(n, tile):
        """Tiles of an item of n raters (numpy int64): C (C + 1) / 2 with C = ceil(n / tile), none below two raters."""
        c = np.where(n < 2, 0, (n + tile - 1) // tile)
        return c * (c + 1) // 2

    def add(self, user, item, dev):
        """Adds the rows (user, item, dev) -- numpy arrays or tensors, any order; ``dev`` from ``rating_deviations``."""
        pairs = self._pairs
        pairs.check_usable()
        user, item, dev = _tensor(user, "user"), _tensor(item, "item"), _tensor(dev, "dev")
        _same_length("user, item and dev", user, item, dev)
        if dev.dtype.is_floating_point or user.dtype.is_floating_point or item.dtype.is_floating_point:
            raise TypeError("user, item and dev must be integer arrays (dev: rating_deviations)")
        if user.numel() == 0:
            return self
        # the two refusals and the launch plan, on the inputs' own device (the host for host inputs): nothing below the
        # plan touches the builder's device when there is nothing to launch
        new_items, counts = torch.unique(item.to(torch.int64), return_counts=True)
        new_items, n = new_items.cpu().numpy(), counts.cpu().numpy().astype(np.int64)
        again = np.intersect1d(new_items, self._items)
        if again.size:
            raise ValueError("item %d was given in an earlier add: all raters of an item must arrive in one add"
                             % int(again[0]))
        m = max(self._max_dev, int(dev.to(torch.int64).abs().max()))
        n_items = int(self._items.size + new_items.size)
        if m * m * n_items >= 1 << 53:
            raise ValueError("exactness bound: max |dev|^2 x items = %d^2 x %d >= 2^53, the sums of squares may not be "
                             "exact in a double; lower frac_bits in rating_deviations" % (m, n_items))
        plan = [r for r in plan_ranges(np.concatenate([[0], np.cumsum(n * (n - 1) // 2)]), self.max_pairs_per_launch)
                if r[2]]
        self._items, self._max_dev = np.union1d(self._items, new_items), m
        self._max_user = max(self._max_user, int(user.max()))
        if not plan:
            return self
        with torch.cuda.device(self.device):
            user = user.to(self.device).to(torch.int64)
            item = item.to(self.device).to(torch.int64)
            order = torch.sort((item << 32) | (user & 0xFFFFFFFF)).indices     # (item, user); a negative user sorts last
            users_s = user[order].to(torch.int32).contiguous()
            dev_s = dev.to(self.device).to(torch.int32)[order].contiguous()
            # CSR by item: the items ascending, as torch.unique listed them
            offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
            tile_prefix = np.concatenate([[0], np.cumsum(self.tiles_of(n, ops.usersim_tile()))]).astype(np.int64)
            off_dev, tp_dev = torch.from_numpy(offsets).to(self.device), torch.from_numpy(tile_prefix).to(self.device)
            ids_dev = torch.from_numpy(np.clip(new_items, -1, 2 ** 31 - 1).astype(np.int32)).to(self.device)
            for a, b, bound in plan:
                pairs.reserve(bound)
                ops.usersim_accumulate(pairs.tensor, pairs.capacity, users_s, dev_s, off_dev, ids_dev, tp_dev, a, b,
                                       int(tile_prefix[b] - tile_prefix[a]))
                self.launches += 1
                pairs.sync()
                pairs.settle()
        return self

    def finalize(self, min_overlap=1, min_similarity=None):
        """(index int32[nnz], other int32[nnz], sim float32[nnz], overlap int32[nnz]) on the device, ascending by (index,
        other) with index < other.  Dropped: entries with Qa == 0 or Qb == 0 (a user whose deviations over the common
        items are all zero; counted in ``dropped_flat``), with overlap < `min_overlap`, and -- when `min_similarity` is
        given (rounded to float32) -- with ``sim <= min_similarity``.  The builder stays usable."""
        min_overlap = int(min_overlap)
        if min_overlap < 1:
            raise ValueError("min_overlap = %d below 1" % min_overlap)
        if min_similarity is not None:
            min_similarity = float(np.float32(min_similarity))
            if min_similarity != min_similarity:
                raise ValueError("min_similarity is NaN")
        pairs = self._pairs
        pairs.check_usable()
        if not pairs.used:
            e = lambda dt: torch.empty(0, dtype=dt, device=self.device)  # noqa: E731
            self.dropped_flat = 0
            return e(torch.int32), e(torch.int32), e(torch.float32), e(torch.int32)
        with torch.cuda.device(self.device):
            index, other, sim, overlap, flat = ops.usersim_finalize(pairs.tensor, pairs.capacity, pairs.used,
                                                                    self._max_user + 1, min_overlap, min_similarity)
            pairs.sync()
        self.dropped_flat = int(flat)
        return index, other, sim, overlap


def max_entries():
    """The ratings of all neighbours that one ``recommend`` query may gather (esr_userknn_max_entries(): a workgroup sorts
    them in LDS)."""
    return ops.userknn_max_entries()


def _check_modes(center, denominator):
    if center not in CENTERS:
        raise ValueError("center must be 'query' or 'neighbour', got %r" % (center,))
    if denominator not in DENOMINATORS:
        raise ValueError("denominator must be 'rated' or 'all', got %r" % (denominator,))
    return center == "neighbour", denominator == "all"


class UserKnn:
    """The user-kNN predictor: a ``NeighbourTable`` over users (``neighbours(index, other, sim, users, None, k,
    orientation="both", score="count")``), the ratings (one per (user, item): ``latest_ratings``; kept as float32) and
    (users, mean) from ``rating_deviations``.  Holds the ratings as CSR by user with the items ascending (the sort is torch
    plumbing).  See the module text for the arithmetic."""

    def __init__(self, table, user, item, rating, users, mean):
        if not isinstance(table.ids, torch.Tensor) or not table.ids.is_cuda:
            raise TypeError("table must hold CUDA/ROCm tensors (no CPU fallback exists)")
        dev = table.ids.device
        user, item, rating = _tensor(user, "user"), _tensor(item, "item"), _tensor(rating, "rating")
        users, mean = _tensor(users, "users"), _tensor(mean, "mean")
        _same_length("user, item and rating", user, item, rating)
        _same_length("users and mean", users, mean)
        self.table, self.device = table, dev
        with torch.cuda.device(dev):
            self.users = ops.as_ids(users.to(dev), dev)
            self.mean = mean.to(device=dev, dtype=torch.float64).contiguous()
            key = (user.to(dev).to(torch.int64) << 32) + item.to(dev).to(torch.int64)
            key, order = torch.sort(key)
            if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
                raise ValueError("a (user, item) is rated twice: keep one rating per pair (latest_ratings)")
            if self.users.numel() > 1 and bool((self.users[1:] <= self.users[:-1]).any()):
                raise ValueError("users must be strictly ascending (rating_deviations)")
            by_user = key >> 32
            lo = torch.searchsorted(by_user, self.users.to(torch.int64))
            hi = torch.searchsorted(by_user, self.users.to(torch.int64), right=True)
            if int((hi - lo).sum()) != key.numel():
                raise ValueError("a rating's user is not in users")
            self.row_offsets = torch.cat([lo, torch.tensor([key.numel()], dtype=torch.int64, device=dev)]).contiguous()
            self.items = (key & 0xFFFFFFFF).to(torch.int32).contiguous()
            self.ratings = rating.to(dev)[order].to(torch.float32).contiguous()

    def _args(self):
        t = self.table
        return (t.ids, t.neighbours, t.scores, t.lengths, self.users, self.row_offsets, self.items, self.ratings, self.mean)

    def predict(self, users, items, center="neighbour", denominator="rated"):
        """(aff float32[nq], support int32[nq]) of the queries (users[q], items[q]); a user the table (or ``users``)
        lacks gets (NaN, 0)."""
        center, den_all = _check_modes(center, denominator)
        users, items = _tensor(users, "users"), _tensor(items, "items")
        _same_length("users and items", users, items)
        with torch.cuda.device(self.device):
            return ops.userknn_predict(*self._args(), ops.as_ids(users.to(self.device), self.device),
                                       ops.as_ids(items.to(self.device), self.device), center, den_all)

    def gathered(self, users):
        """int64[nq] on the device: the ratings a ``recommend`` query of each user gathers -- the sum of its neighbours'
        row lengths (index arithmetic in torch)."""
        t = self.table
        q = ops.as_ids(_tensor(users, "users").to(self.device), self.device).to(torch.int64)
        if t.ids.numel() == 0 or self.users.numel() == 0:
            return torch.zeros(q.numel(), dtype=torch.int64, device=self.device)
        ids = t.ids.to(torch.int64)
        row = torch.searchsorted(ids, q).clamp(max=ids.numel() - 1)
        known = ids[row] == q
        nb = t.neighbours[row].to(torch.int64)                               # [nq, W]
        live = (torch.arange(t.k, device=self.device)[None, :] < t.lengths[row][:, None]) & known[:, None] & (nb >= 0)
        all_users = self.users.to(torch.int64)
        pos = torch.searchsorted(all_users, nb).clamp(max=all_users.numel() - 1)
        live &= all_users[pos] == nb
        lens = self.row_offsets[1:] - self.row_offsets[:-1]
        return (lens[pos] * live).sum(1)

    def recommend(self, users, k, exclude_rated=True, min_support=1, center="neighbour", denominator="rated"):
        """Per query user the k best items among those rated by any of its neighbours -- without the user's own items
        when `exclude_rated`, without those of support below `min_support` -- ordered by affinity descending, then item
        id ascending: (rec_ids int32[nq, k] padded with -1, rec_scores float32[nq, k] padded with 0, rec_lengths
        int32[nq]), the shape ``neighbours.recommend`` returns.  A score equals ``predict`` of the same (user, item) bit
        for bit.  A user the table lacks gets an empty list.

        A query gathers the sum of its neighbours' row lengths, at most ``max_entries()``; a larger one raises
        ``ValueError`` naming the query before any launch and is never truncated."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
        min_support = int(min_support)
        if min_support < 0:
            raise ValueError("min_support = %d is negative" % min_support)
        center, den_all = _check_modes(center, denominator)
        users = _tensor(users, "users")
        with torch.cuda.device(self.device):
            users = ops.as_ids(users.to(self.device), self.device)
            gathered = self.gathered(users)
            cap = max_entries()
            over = torch.nonzero(gathered > cap).reshape(-1)
            if over.numel():
                q = int(over[0])
                raise ValueError("query %d (user %d) gathers %d ratings from its neighbours, above the cap of %d per query "
                                 "(esr_ratings.hip sorts a query in LDS); build a narrower table"
                                 % (q, int(users[q]), int(gathered[q]), cap))
            return ops.userknn_recommend(*self._args(), users, k, exclude_rated, min_support, center, den_all)

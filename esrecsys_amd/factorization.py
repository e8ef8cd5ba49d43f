"""Matrix factorisation of explicit ratings by alternating least squares on the GPU (esr_als.hip): the low-rank model the
reference's book turns to after the neighbourhood methods of ``ratings.py``.

    user, item, rating = latest_ratings(user, item, rating, tstamp)
    model = RatingsALS(user, item, rating, rank=32, reg=0.1)
    history = model.fit(sweeps=10)                    # the objective after every half-sweep (2 per sweep)
    pred = model.predict(users, items)                # NaN where the user or the item is unknown
    rec_ids, rec_scores, rec_lengths = model.recommend(users, k=500)     # straight into evaluate.ranking_metrics

Model.  ``r^[u, i] = c[u] + x_u . y_i``; the offset c[u] is the user's mean (``center="user"``, the mean of
``rating_deviations``, which the kNN path also centres on), the global mean (``"global"``: an fp64 torch sum divided by the
count) or 0 (``"none"``).  The fitted targets are ``d[u, i] = float32(float64(r) - c[u])``.

Objective.  ``J = sum (d - x_u . y_i)^2 + reg sum_u w_u |x_u|^2 + reg sum_i w_i |y_i|^2`` with w = the row's rating count
(``weighted_reg``, weighted-lambda: the default) or 1.

Half-sweep.  Every row u with n ratings solves ``(sum_k y_k y_k^T + lam I) x_u = sum_k d_k y_k``, ``lam = reg * (n if
weighted_reg else 1)``, in ONE kernel call (``ops.als_solve_rows``); the item half-sweep is the same call on the transposed
CSR.  A row without ratings gets the zero vector.  The Gram matrix runs on the exact-f32 MFMA in a fixed order (per chunk of
``ops.als_geometry()[0]`` consecutive ratings a k-ordered fmaf chain, chunk partials added in ascending order), followed by
an f32 Cholesky: a row's solution depends on its own ratings, the other side's factors, reg and weighted_reg only, so the fit
is a function of the inputs and the seed -- not of the grid or of ``max_rows_per_launch``.

Prediction.  One kernel computes ``float32(c[u] + sum_d float64(x[d]) * float64(y[d]))`` (fp64, ascending d, rounded once);
``residuals`` is ``float32(float64(d) - dot)`` by the same kernel; ``objective`` and ``rmse`` are fp64 torch reductions
over those outputs and the factor tables.

Implicit feedback.  ``ImplicitALS`` (below) is the confidence-weighted model of Hu, Koren and Volinsky for occurrence data:
every cell is fitted, a half-sweep is one ``ops.als_gram`` and one ``ops.als_solve_rows_implicit``, and new documents are
folded in by the same call (``fold_in``, ``recommend_documents``).  ``BPR`` (further below) is the model of the same family
that is trained on the ranking itself: Bayesian Personalised Ranking over triples sampled on the device (esr_bpr.hip), updated
by the row-sparse engine; ``WARP`` (last) is BPR's model trained with the rank-weighted margin loss, its negatives searched
for on the device by one fused call (esr_warp.hip).  ``HybridBPR`` is BPR over users and items that are weighted sums of
feature embeddings (esr_bag.hip): side information and cold start.  ``FPMC`` (at the end) is the sequential member: BPR's
user-item term plus a factorised transition term from the items just consumed (esr_fpmc.hip), which also serves sessions of
users the model never saw.  ``SGNS`` (the last class) has no users at all: skip-gram with negative sampling over id sequences
(esr_sgns.hip) -- word2vec, item2vec.

All of them derive from ``_Factorization`` (device, indexed pairs, ``score`` / ``recommend`` / ``from_documents`` and
``diversify``, the MMR re-ranking of ``rerank.py`` applied to ``recommend``'s lists); ``_ALS`` holds
what the two alternating models share, ``_SampledSGD`` what the five models trained by sampled SGD share (the
hyper-parameters, the seeded tables, the row-sparse update, the tail of ``train_steps``, ``fit``); ``BPR`` adds the seen
pairs and the triple step that ``WARP``, ``HybridBPR`` and ``FPMC`` build on, and ``_Sequences`` holds the event CSR and
the serving of given sequences for ``FPMC`` and ``SGNS``.
"""
import math

import numpy as np
import torch

from . import ops
from .ratings import _same_length, _tensor, rating_deviations
from .wikipedia.neighbours import MAX_K

CENTERS = ("user", "global", "none")
RETRIEVE_LIMIT = 1024        # the k of ops.retrieve_topk
FAIL_BAD_POSITION = 1 << 30  # esr_als.hip, esr_bpr.hip, esr_warp.hip, esr_bag.hip: a position outside its table
FAIL_BAD_WEIGHT = 1 << 29    # esr_als.hip: a weight that is negative or not finite


class FactorizationError(RuntimeError):
    """A half-sweep could not solve some rows (a pivot that is not finite and positive: NaN factors handed in), or met a
    column outside the other side's table."""


def max_rank():
    """The largest rank the kernels take (esr_als_max_rank(): one wave holds a rank x rank f32 matrix in LDS)."""
    return ops.als_max_rank()


def predict_max_rank():
    """The widest row ``score``, ``recommend`` and ``diversify`` take (esr_als_predict_max_rank(): the predict kernel is a
    per-pair loop, so its cap is the row-group cap of ``ops.bpr_geometry()``, above ``max_rank()``)."""
    return ops.als_predict_max_rank()


def _raise_failed(word, side):
    """The failure word of a row solve as a ``FactorizationError``: bit 30, bit 29, else the count of unsolved rows."""
    if word & FAIL_BAD_POSITION:
        raise FactorizationError("the %s half-sweep met a position outside the other side's table" % side)
    if word & FAIL_BAD_WEIGHT:
        raise FactorizationError("the %s half-sweep met a weight that is negative or not finite (bit 29)" % side)
    if word:
        raise FactorizationError("the %s half-sweep could not solve %d row(s): a pivot that is not finite and positive "
                                 "(are the other side's factors finite?); those rows were left unchanged" % (side, word))


def _host_offsets(counts):
    """Contiguous host int64[n + 1]: 0 and the running sums of `counts` (a tensor or an array)."""
    if isinstance(counts, torch.Tensor):
        counts = counts.cpu().numpy()
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).astype(np.int64))


def _csr(major, minor, n_major):
    """(host row offsets int64[n_major + 1], order): the rows sorted by (major, minor) -- torch plumbing."""
    key = (major.to(torch.int64) << 32) | minor.to(torch.int64)
    key, order = torch.sort(key)
    return key, _host_offsets(torch.bincount(major.to(torch.int64), minlength=n_major)), order


def _ids_and_offsets(indices, doc_offsets, dev):
    """(ids int64 on `dev`, host offsets int64[ndocs + 1]) of an id-document CSR given as host arrays or tensors."""
    ids = _tensor(indices, "indices")
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise TypeError("indices must be an integer array")
    off = doc_offsets.detach().cpu().numpy() if isinstance(doc_offsets, torch.Tensor) else np.asarray(doc_offsets)
    if off.dtype.kind not in "iu":
        raise TypeError("doc_offsets must be an integer array")
    off = np.ascontiguousarray(off.reshape(-1).astype(np.int64))
    ids = ids.reshape(-1).to(dev).to(torch.int64)
    if off.size < 1 or int(off[0]) != 0 or int(off[-1]) != ids.numel() or bool((np.diff(off) < 0).any()):
        raise ValueError("doc_offsets must ascend from 0 to the %d ids of indices" % ids.numel())
    return ids, off


class _Factorization:
    """What the six models share (the module text).  A subclass provides ``user_factors`` / ``item_factors``."""

    def _set_device(self, user, item, device):
        """The last two refusals of every constructor that need no device work: integer ids, a CUDA device."""
        if user.dtype.is_floating_point or item.dtype.is_floating_point:
            raise TypeError("user and item must be integer arrays")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA/ROCm device (no CPU fallback exists)")

    def _index_pairs(self, user, item):
        """``users`` / ``items`` (int32 ascending) of the raw ids; returns (user int64 on the device, upos, ipos int64)."""
        user, item = user.to(self.device).to(torch.int64), item.to(self.device).to(torch.int64)
        if user.numel() and (int(user.min()) < 0 or int(item.min()) < 0 or int(user.max()) >= 2 ** 31 - 1
                             or int(item.max()) >= 2 ** 31 - 1):
            raise ValueError("user and item ids must lie in [0, 2^31 - 1)")
        users, upos = torch.unique(user, return_inverse=True)
        items, ipos = torch.unique(item, return_inverse=True)
        self.users, self.items = users.to(torch.int32).contiguous(), items.to(torch.int32).contiguous()
        self._failed = torch.zeros(1, dtype=torch.int32, device=self.device)     # the failure word of every kernel call
        return user, upos, ipos

    def _set_pairs(self, key, user_offsets):
        """The CSR by user of the distinct pairs: `key` = upos << 32 | ipos ascending, its host row offsets."""
        self._key, self._user_offsets = key, user_offsets
        self._row_upos = (key >> 32).to(torch.int32).contiguous()
        self._row_ipos = (key & 0xFFFFFFFF).to(torch.int32).contiguous()

    def _raise_bad_position(self, what):
        """Reads the failure word; bit 30 raises ``FactorizationError(what)``."""
        if int(self._failed.item()) & FAIL_BAD_POSITION:
            raise FactorizationError(what)

    @classmethod
    def from_documents(cls, indices, doc_offsets, **kw):
        """The model of id documents ``indices[doc_offsets[d]:doc_offsets[d + 1]]``: the user is the document number.  An id
        repeated within d is a repeated event: ``ImplicitALS`` adds the strengths (without `strength`: the id's occurrence
        count in d), ``BPR`` and its subclasses keep one seen pair; ``FPMC`` also keeps d's ids as a sequence in order."""
        ids, off = _ids_and_offsets(indices, doc_offsets, torch.device("cpu"))
        docs = torch.from_numpy(np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off)))
        return cls(docs, ids, **kw)

    def _positions(self, ids, table):
        """int32 positions of `ids` in the ascending `table`, -1 where absent.  The ids are compared as int64: one that does
        not fit int32 is absent, never wrapped onto a known id."""
        ids = _tensor(ids, "ids")
        if ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise TypeError("ids must be an integer array")
        ids = ids.to(self.device).to(torch.int64).contiguous()
        if table.numel() == 0:
            return torch.full_like(ids, -1, dtype=torch.int32)
        t = table.to(torch.int64)
        pos = torch.searchsorted(t, ids).clamp(max=t.numel() - 1)
        return torch.where(t[pos] == ids, pos, torch.full_like(pos, -1)).to(torch.int32).contiguous()

    def _rows(self):
        """(query table [nu, width], item table [ni, width]): the rows whose dot product is the model's score -- what
        ``score``, ``recommend`` and ``diversify`` read."""
        return self.user_factors, self.item_factors

    def _score(self, users, items, offset=None):
        users, items = _tensor(users, "users"), _tensor(items, "items")
        _same_length("users and items", users, items)
        with torch.cuda.device(self.device):
            queries, rows = self._rows()
            return ops.als_predict(queries, rows, self._positions(users, self.users), self._positions(items, self.items),
                                   offset=offset)

    def score(self, users, items):
        """float32[nq]: ``float32(x_u . y_i)`` (fp64 sum in ascending dimension); NaN where the user or the item is
        unknown."""
        return self._score(users, items)

    def _recommend(self, users, k, slack, exclude, verb="has seen", flag="exclude_seen", offset=None):
        with torch.cuda.device(self.device):
            upos = self._positions(users, self.users).to(torch.int64)
            queries, rows = self._rows()
            return _recommend_rows(queries, offset, upos, rows, self.items, k, slack,
                                   self._user_offsets if exclude else None, self._key,
                                   lambda q: "user %d" % int(_tensor(users, "users")[q]), verb, flag)

    def recommend(self, users, k=500, exclude_seen=True, slack=16):
        """Per query user the k best items by (score descending, item id ascending), without the user's seen items when
        `exclude_seen`: (rec_ids int32[nq, k] padded with -1, rec_scores float32[nq, k] padded with 0, rec_lengths
        int32[nq]) as ``RatingsALS.recommend``, by the same candidate scheme; a score equals ``score`` of the pair bit for
        bit, an unknown user gets an empty list."""
        return self._recommend(users, k, slack, exclude_seen)

    def diversify(self, rec_ids, rec_scores, rec_lengths, lam=0.7, n=None, normalize=True):
        """The lists of ``recommend`` (device tensors) re-ranked by Maximal Marginal Relevance (``rerank.mmr``): per query
        the n (default: the lists' width) picks that trade a candidate's score (weight lam) against its greatest similarity
        to the items picked before it (weight 1 - lam).  The similarity is the dot product of the items' factor rows
        (``item_rows()`` for ``HybridBPR``), of unit length when `normalize`: the cosine.  Returns (rec_ids, rec_scores,
        rec_lengths) in ``recommend``'s shape and padding, in pick order; ``lam = 1`` keeps ``recommend``'s order.  An id
        inside a list's length that is no item of the model raises ``ValueError``."""
        from . import rerank
        ops._req(rec_ids, torch.int32, "rec_ids"), ops._req(rec_scores, torch.float32, "rec_scores")
        if rec_ids.dim() != 2 or rec_scores.shape != rec_ids.shape:
            raise ValueError("rec_ids and rec_scores must be [nq, width] alike")
        nq, width = rec_ids.shape
        with torch.cuda.device(self.device):
            pos = self._positions(rec_ids.reshape(-1), self.items).reshape(nq, width)
            inside = torch.arange(width, device=self.device)[None, :] < \
                (rec_lengths.to(torch.int64)[:, None] if rec_lengths is not None else width)
            unknown = inside & (pos < 0)
            if bool(unknown.any()):
                q, c = (int(v) for v in unknown.nonzero()[0])
                raise ValueError("query %d: id %d at place %d of its list is not an item of the model"
                                 % (q, int(rec_ids[q, c]), c))
            rows = self._rows()[1]
            rows = rerank.unit_rows(rows) if normalize else rows.contiguous()
            items, rel, lengths, _, _ = rerank.mmr(pos, rec_scores, rec_lengths, rows, lam, n)
            ids = torch.where(items >= 0, self.items[items.clamp(min=0).to(torch.int64)], torch.full_like(items, -1))
        return ids, rel, lengths


def _recommend_rows(factors, offset, upos, item_factors, items, k, slack, seen_offsets, seen_key, name, verb, flag):
    """The body every ``recommend`` and ``ImplicitALS.recommend_documents`` share.  Query q is row ``upos[q]`` (int64, -1:
    unknown, an empty list) of ``factors``; its score of item position i is ``ops.als_predict`` of that pair with ``offset``
    (float64 per row, or None).  With ``seen_offsets`` (host CSR offsets of the rows' own items) the pairs of ``seen_key``
    (``row << 32 | item position``, ascending) are left out.  ``name(q)``, ``verb`` and ``flag`` word the refusal of a query
    with too many candidates."""
    k, slack = int(k), int(slack)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
    if slack < 0:
        raise ValueError("slack = %d is negative" % slack)
    dev = factors.device
    exclude = seen_offsets is not None
    nq, ni = int(upos.numel()), int(items.numel())
    ids = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
    scores = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    lengths = torch.zeros(nq, dtype=torch.int32, device=dev)
    if nq == 0 or ni == 0:
        return ids, scores, lengths
    known = upos >= 0
    safe = upos.clamp(min=0)
    r_max = 0
    if exclude and bool(known.any()):
        lens = torch.from_numpy(np.diff(seen_offsets)).to(dev)
        rated = torch.where(known, lens[safe], torch.zeros_like(safe))
        r_max = int(rated.max())
        if k + r_max + slack > RETRIEVE_LIMIT and ni > RETRIEVE_LIMIT:
            q = int(torch.argmax(rated))
            raise ValueError("query %d (%s) %s %d items: k + rated + slack = %d candidates exceed the %d "
                             "that retrieve_topk selects; lower k or query that user without %s"
                             % (q, name(q), verb, r_max, k + r_max + slack, RETRIEVE_LIMIT, flag))
    kc = min(ni, k + r_max + slack)
    if kc > RETRIEVE_LIMIT:
        raise ValueError("query 0: k + slack = %d candidates exceed the %d that retrieve_topk selects"
                         % (k + slack, RETRIEVE_LIMIT))
    queries = torch.where(known[:, None], factors[safe], torch.zeros((), device=dev)).contiguous()
    _, cand = ops.retrieve_topk(queries, item_factors, kc, mode="exact")          # [nq, kc] item positions
    cand = cand.to(torch.int64)
    sc = ops.als_predict(factors, item_factors, upos[:, None].expand(nq, kc).to(torch.int32).contiguous().reshape(-1),
                         cand.to(torch.int32).contiguous().reshape(-1), offset=offset).reshape(nq, kc)
    drop = ~known[:, None].expand(nq, kc)
    if exclude and seen_key.numel():
        pair = (safe[:, None] << 32) | cand
        at = torch.searchsorted(seen_key, pair.reshape(-1)).clamp(max=seen_key.numel() - 1).reshape(nq, kc)
        drop = drop | (seen_key[at] == pair)
    # (score descending, item ascending): positions ascend with ids; dropped candidates go last
    by_item = torch.sort(cand, dim=1, stable=True)
    sc_i, drop_i = torch.gather(sc, 1, by_item.indices), torch.gather(drop, 1, by_item.indices)
    rank_key = torch.where(drop_i, torch.full_like(sc_i, -float("inf")), sc_i)
    by_score = torch.sort(rank_key, dim=1, descending=True, stable=True)
    live = (~torch.gather(drop_i, 1, by_score.indices))[:, :k]
    kk = min(k, kc)
    top_items = torch.gather(by_item.values, 1, by_score.indices)[:, :kk]
    top_scores = torch.gather(sc_i, 1, by_score.indices)[:, :kk]
    ids[:, :kk] = torch.where(live, items[top_items], torch.full_like(ids[:, :kk], -1))
    scores[:, :kk] = torch.where(live, top_scores, torch.zeros_like(top_scores))
    lengths = live.sum(1).to(torch.int32)
    return ids, scores, lengths


# ---- the two alternating models --------------------------------------------------------------------------------------------
class _ALS(_Factorization):
    """What ``RatingsALS`` and ``ImplicitALS`` share.  A subclass provides ``_solve_slice``, ``solve_users`` / ``solve_items``
    and ``objective``."""

    @staticmethod
    def _check_rank_reg(rank, reg, why=""):
        rank = int(rank)
        if not 1 <= rank <= max_rank():
            raise ValueError("rank = %d outside [1, %d]" % (rank, max_rank()))
        reg = float(reg)
        if not (math.isfinite(reg) and reg > 0.0 and float(np.float32(reg)) > 0.0 and math.isfinite(float(np.float32(reg)))):
            raise ValueError("reg = %r must be finite and positive%s" % (reg, why))
        return rank, reg

    @staticmethod
    def _check_rows_per_launch(max_rows_per_launch):
        if max_rows_per_launch is not None and int(max_rows_per_launch) < 1:
            raise ValueError("max_rows_per_launch = %r below 1" % (max_rows_per_launch,))
        return None if max_rows_per_launch is None else int(max_rows_per_launch)

    def _configure(self, user, item, device, rank, reg, weighted_reg, seed, init_scale, max_rows_per_launch):
        self._set_device(user, item, device)
        self.rank, self.reg, self.weighted_reg, self.seed = rank, reg, bool(weighted_reg), int(seed)
        self.max_rows_per_launch = max_rows_per_launch
        self.init_scale = float(rank) ** -0.5 if init_scale is None else float(init_scale)

    def _by_item(self, values):
        """The transposed CSR (``_item_offsets``, ``_col_upos``: users ascending within an item); returns `values` (one
        per pair, in CSR-by-user order) in its order."""
        _, self._item_offsets, order_i = _csr(self._row_ipos, self._row_upos, int(self.items.numel()))
        self._col_upos = self._row_upos[order_i].contiguous()
        return values[order_i].contiguous()

    def _init_factors(self):
        """``item_factors = randn * init_scale`` from the seeded CPU generator (the only draw), ``user_factors = 0``."""
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        self.item_factors = (torch.randn(int(self.items.numel()), self.rank, generator=gen)
                             * self.init_scale).to(self.device).contiguous()
        self.user_factors = torch.zeros(int(self.users.numel()), self.rank, dtype=torch.float32, device=self.device)

    def _half_sweep(self, side, other, offsets, cols, values, out, gram=None):
        """``_solve_slice`` (the subclass's one kernel call) per ``max_rows_per_launch`` slice, then the failure word."""
        n_rows = offsets.size - 1
        step = n_rows if self.max_rows_per_launch is None else self.max_rows_per_launch
        with torch.cuda.device(self.device):
            self._failed.zero_()
            for a in range(0, n_rows, max(step, 1)):
                self._solve_slice(other, gram, offsets, cols, values, a, min(a + step, n_rows), out)
            word = int(self._failed.item())
        _raise_failed(word, side)

    def sweep(self):
        """One user half-sweep, then one item half-sweep."""
        self.solve_users()
        self.solve_items()

    def fit(self, sweeps=10):
        """`sweeps` sweeps; returns the objective after every half-sweep (2 per sweep), a list of float."""
        history = []
        for _ in range(int(sweeps)):
            self.solve_users()
            history.append(self.objective())
            self.solve_items()
            history.append(self.objective())
        return history

    def _reg_terms(self, X, Y):
        """(reg sum_u w_u |x_u|^2, reg sum_i w_i |y_i|^2) of the fp64 tables X, Y: w the row's pair count or 1."""
        wu = torch.from_numpy(np.diff(self._user_offsets)).to(self.device).to(torch.float64)
        wi = torch.from_numpy(np.diff(self._item_offsets)).to(self.device).to(torch.float64)
        if not self.weighted_reg:
            wu, wi = torch.ones_like(wu), torch.ones_like(wi)
        return self.reg * (wu * (X ** 2).sum(1)).sum(), self.reg * (wi * (Y ** 2).sum(1)).sum()


class RatingsALS(_ALS):
    """See the module text.  ``users`` / ``items``: int32 ascending ids; ``user_factors`` / ``item_factors``: float32
    [nu, rank] / [ni, rank]; ``user_mean``: float64[nu], the offset c."""

    def __init__(self, user, item, rating, rank=32, reg=0.1, weighted_reg=True, center="user", seed=0, init_scale=None,
                 device=None, max_rows_per_launch=None):
        rank, reg = self._check_rank_reg(rank, reg, " (a row with fewer ratings than rank is singular without it)")
        if center not in CENTERS:
            raise ValueError("center must be 'user', 'global' or 'none', got %r" % (center,))
        max_rows_per_launch = self._check_rows_per_launch(max_rows_per_launch)
        user, item, rating = _tensor(user, "user"), _tensor(item, "item"), _tensor(rating, "rating")
        _same_length("user, item and rating", user, item, rating)
        self._configure(user, item, device, rank, reg, weighted_reg, seed, init_scale, max_rows_per_launch)
        self.center = center
        dev = self.device
        with torch.cuda.device(dev):
            rating64 = rating.to(device=dev, dtype=torch.float64)
            user, upos, ipos = self._index_pairs(user, item)
            nu = int(self.users.numel())
            if center == "user":
                _, mean, _ = rating_deviations(user, rating64, frac_bits=0)
            elif center == "global":
                # (divided on the host: a tensor divided by a scalar is multiplied by its reciprocal on the device)
                g = float(rating64.sum()) / rating64.numel() if rating64.numel() else 0.0
                mean = torch.full((nu,), g, dtype=torch.float64, device=dev)
            else:
                mean = torch.zeros(nu, dtype=torch.float64, device=dev)
            self.user_mean = mean.contiguous()
            d = (rating64 - self.user_mean[upos]).to(torch.float32)
            # CSR by user (items ascending) and by item (users ascending)
            key, user_offsets, order = _csr(upos, ipos, nu)
            if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
                raise ValueError("a (user, item) is rated twice: keep one rating per pair (latest_ratings)")
            self._set_pairs(key, user_offsets)                          # the training pairs
            self._targets = d[order].contiguous()
            self._targets_by_item = self._by_item(self._targets)
            self._init_factors()

    nnz = property(lambda self: int(self._targets.numel()))

    # ---- the fit --------------------------------------------------------------------------------------------------------
    def _solve_slice(self, other, gram, offsets, cols, targets, a, b, out):
        ops.als_solve_rows(other, offsets, cols, targets, a, b, self.reg, self.weighted_reg, out, self._failed)

    def solve_users(self):
        self._half_sweep("user", self.item_factors, self._user_offsets, self._row_ipos, self._targets, self.user_factors)

    def solve_items(self):
        self._half_sweep("item", self.user_factors, self._item_offsets, self._col_upos, self._targets_by_item,
                         self.item_factors)

    # ---- prediction -----------------------------------------------------------------------------------------------------
    def predict(self, users, items):
        """float32[nq]: ``float32(c[u] + x_u . y_i)``; NaN where the user or the item is unknown."""
        return self._score(users, items, offset=self.user_mean)

    def residuals(self):
        """float32[nnz]: ``float32(float64(d) - x_u . y_i)`` of the training pairs in CSR-by-user order."""
        with torch.cuda.device(self.device):
            return ops.als_predict(self.user_factors, self.item_factors, self._row_upos, self._row_ipos, targets=self._targets)

    def objective(self):
        """J of the module text, an fp64 reduction (python float)."""
        with torch.cuda.device(self.device):
            res = self.residuals().to(torch.float64)
            reg_u, reg_i = self._reg_terms(self.user_factors.to(torch.float64), self.item_factors.to(torch.float64))
            return float((res * res).sum() + reg_u + reg_i)

    def rmse(self, users, items, ratings):
        """Root mean squared error of ``predict`` over the pairs both of whose ids are known (NaN when there is none)."""
        ratings = _tensor(ratings, "ratings").to(device=self.device, dtype=torch.float64)
        pred = self.predict(users, items).to(torch.float64)
        known = ~torch.isnan(pred)
        if not bool(known.any()):
            return float("nan")
        e = pred[known] - ratings[known]
        return float(torch.sqrt((e * e).sum() / e.numel()))

    # ---- recommendation ---------------------------------------------------------------------------------------------------
    def recommend(self, users, k=500, exclude_rated=True, slack=16):
        """Per query user the k best items by (score descending, item id ascending), without the user's own items when
        `exclude_rated`: (rec_ids int32[nq, k] padded with -1, rec_scores float32[nq, k] padded with 0, rec_lengths
        int32[nq]), the shape ``UserKnn.recommend`` returns.  A score equals ``predict`` of the same pair bit for bit; an
        unknown user gets an empty list.

        Candidates are ``ops.retrieve_topk(x_u, item_factors, k', mode="exact")`` with ``k' = min(ni, k + r_max + slack)``,
        r_max the longest rated list among the queried users (0 without `exclude_rated`); they are re-scored by the predict
        kernel.  A k' above retrieve_topk's limit raises ``ValueError`` naming the query before any launch."""
        return self._recommend(users, k, slack, exclude_rated, "rated", "exclude_rated", offset=self.user_mean)


# ---- implicit feedback ---------------------------------------------------------------------------------------------------
def _sum_events(major, minor, strength, n_major, alpha):
    """Events (major, minor, strength float64) with repeats -> (key int64 ascending and distinct, major << 32 | minor; host
    row offsets int64[n_major + 1]; w float32 = float32(alpha * the pair's strengths summed in fp64 in the events' order)).
    The sum runs over a stable sort on the host (numpy add.reduceat): the same bits for the same events, whatever the
    device did before -- torch plumbing, not a hot path."""
    dev = major.device
    key = (major.to(torch.int64) << 32) | minor.to(torch.int64)
    key, order = torch.sort(key, stable=True)
    ukey, counts = torch.unique_consecutive(key, return_counts=True)
    if key.numel():
        starts = (torch.cumsum(counts, 0) - counts).cpu().numpy()
        sums = np.add.reduceat(strength[order].cpu().numpy().astype(np.float64), starts)
    else:
        sums = np.zeros(0, np.float64)
    w = (np.float64(alpha) * sums).astype(np.float32)
    return ukey, _host_offsets(torch.bincount(ukey >> 32, minlength=n_major)), torch.from_numpy(w).to(dev)


class ImplicitALS(_ALS):
    """Confidence-weighted matrix factorisation of implicit feedback (Hu, Koren, Volinsky 2008) by ALS on the GPU.

        model = ImplicitALS.from_documents(indices, doc_offsets, rank=32, alpha=40.0)   # user = document, strength = count
        history = model.fit(sweeps=10)                     # the full-matrix objective after every half-sweep
        x = model.fold_in(new_indices, new_offsets)        # factors of NEW documents against the fitted items, no retraining
        rec_ids, rec_scores, rec_lengths = model.recommend_documents(context, context_offsets, k=500)

    Model.  EVERY (user, item) cell is fitted: preference p = 1 where the pair was seen and 0 elsewhere, confidence
    ``c = 1 + w`` with ``w = float32(alpha * strength)`` on the seen cells (repeated events add their strengths in fp64) and
    1 on the rest.

    Objective.  ``J = sum over ALL cells of c (p - x_u . y_i)^2 + reg (sum_u w_u |x_u|^2 + sum_i w_i |y_i|^2)``, w the
    row's number of seen cells (``weighted_reg``) or 1 (the default).

    Half-sweep.  One ``ops.als_gram`` of the other side (``G = Y^T Y``) and one ``ops.als_solve_rows_implicit`` per
    ``max_rows_per_launch`` slice: a row with n seen cells solves ``(G + sum_k w_k y_k y_k^T + lam I) x = sum_k (1 + w_k)
    y_k``, ``lam = reg * (n if weighted_reg else 1)``, in the order esr_als.hip states.  A solved row is a function of its
    own (item, weight) list, the other side's factors, reg and weighted_reg alone, so ``fold_in`` of a training user's own
    items returns that user's row bit for bit.  A row without seen cells gets the zero vector."""

    def __init__(self, user, item, strength=None, rank=32, reg=0.01, alpha=40.0, weighted_reg=False, seed=0, init_scale=None,
                 device=None, max_rows_per_launch=None):
        rank, reg = self._check_rank_reg(rank, reg)
        alpha = float(alpha)
        if not (math.isfinite(alpha) and alpha > 0.0):
            raise ValueError("alpha = %r must be finite and positive" % (alpha,))
        max_rows_per_launch = self._check_rows_per_launch(max_rows_per_launch)
        user, item = _tensor(user, "user"), _tensor(item, "item")
        if strength is None:
            _same_length("user and item", user, item)
        else:
            strength = _tensor(strength, "strength")
            _same_length("user, item and strength", user, item, strength)
        self._configure(user, item, device, rank, reg, weighted_reg, seed, init_scale, max_rows_per_launch)
        self.alpha = alpha
        with torch.cuda.device(self.device):
            user, upos, ipos = self._index_pairs(user, item)
            s64 = self._strengths(strength, user.numel())
            # CSR by user (items ascending) and its transpose (users ascending); one weight per distinct pair
            key, user_offsets, w = _sum_events(upos, ipos, s64, int(self.users.numel()), alpha)
            if w.numel() and not bool(torch.isfinite(w).all()):
                raise ValueError("alpha * strength does not fit a float32")
            self._set_pairs(key, user_offsets)                          # the seen pairs
            self._weights = w.contiguous()
            self._weights_by_item = self._by_item(self._weights)
            self._init_factors()
            self._item_gram = None      # (Y^T Y, the version of item_factors it was made from): fold_in's cache

    def _strengths(self, strength, n):
        """float64[n] on the device: 1 per event without `strength`; refuses one that is not finite and positive."""
        if strength is None:
            return torch.ones(n, dtype=torch.float64, device=self.device)
        s64 = strength.reshape(-1).to(device=self.device, dtype=torch.float64)
        if s64.numel() and not bool((torch.isfinite(s64) & (s64 > 0)).all()):
            raise ValueError("every strength must be finite and positive")
        return s64

    nnz = property(lambda self: int(self._weights.numel()))

    # ---- the fit --------------------------------------------------------------------------------------------------------
    def _solve_slice(self, other, gram, offsets, cols, weights, a, b, out):
        ops.als_solve_rows_implicit(other, gram, offsets, cols, weights, a, b, self.reg, self.weighted_reg, out, self._failed)

    def _gram_of_items(self):
        """Y^T Y of the item factors, kept until they next change (solve_items, or an in-place torch write)."""
        version = (self.item_factors._version, self.item_factors.data_ptr())
        if self._item_gram is None or self._item_gram[1] != version:
            with torch.cuda.device(self.device):
                self._item_gram = (ops.als_gram(self.item_factors), version)
        return self._item_gram[0]

    def solve_users(self):
        self._half_sweep("user", self.item_factors, self._user_offsets, self._row_ipos, self._weights, self.user_factors,
                         gram=self._gram_of_items())

    def solve_items(self):
        with torch.cuda.device(self.device):
            gram = ops.als_gram(self.user_factors)
        self._item_gram = None
        self._half_sweep("item", self.user_factors, self._item_offsets, self._col_upos, self._weights_by_item,
                         self.item_factors, gram=gram)

    def objective(self):
        """J of the class text in fp64 torch (python float), without the matrix: the cells at confidence 1 and preference 0
        sum to ``sum_u x_u^T (Y^T Y) x_u``; a seen cell with dot s adds ``(1 + w) (1 - s)^2 - s^2``."""
        with torch.cuda.device(self.device):
            X, Y = self.user_factors.to(torch.float64), self.item_factors.to(torch.float64)
            everything = ((X @ (Y.t() @ Y)) * X).sum()
            u, i = self._row_upos.to(torch.int64), self._row_ipos.to(torch.int64)
            s = (X[u] * Y[i]).sum(1)
            c = 1.0 + self._weights.to(torch.float64)
            seen = (c * (1.0 - s) ** 2 - s * s).sum()
            reg_u, reg_i = self._reg_terms(X, Y)
            return float(everything + seen + reg_u + reg_i)

    # ---- new documents ------------------------------------------------------------------------------------------------------
    def _fold_in(self, indices, doc_offsets, strengths):
        ids, off = _ids_and_offsets(indices, doc_offsets, self.device)
        ndocs = off.size - 1
        with torch.cuda.device(self.device):
            if strengths is not None:
                strengths = _tensor(strengths, "strengths")
                if strengths.numel() != ids.numel():
                    raise ValueError("strengths must hold one value per id")
            s64 = self._strengths(strengths, ids.numel())
            docs = torch.from_numpy(np.repeat(np.arange(ndocs, dtype=np.int64), np.diff(off))).to(self.device)
            ipos = self._positions(ids, self.items).to(torch.int64)
            known = ipos >= 0                                            # ids unknown to the model are dropped
            key, offsets, w = _sum_events(docs[known], ipos[known], s64[known], ndocs, self.alpha)
            if w.numel() and not bool(torch.isfinite(w).all()):
                raise ValueError("alpha * strength does not fit a float32")
            out = torch.zeros(ndocs, self.rank, dtype=torch.float32, device=self.device)
            if ndocs:
                self._failed.zero_()
                ops.als_solve_rows_implicit(self.item_factors, self._gram_of_items(), offsets,
                                            (key & 0xFFFFFFFF).to(torch.int32).contiguous(), w.contiguous(), 0, ndocs,
                                            self.reg, self.weighted_reg, out, self._failed)
                _raise_failed(int(self._failed.item()), "fold-in")
            return out, key, offsets

    def fold_in(self, indices, doc_offsets, strengths=None):
        """float32[ndocs, rank]: the user factors of NEW id documents against the fitted item factors -- one Gram (kept until
        the item factors change) and one row-solve call, no retraining.  Ids the model does not know are dropped, a
        repeated id adds its strengths (its count without `strengths`); a document without a known id gets zeros."""
        return self._fold_in(indices, doc_offsets, strengths)[0]

    def recommend_documents(self, indices, doc_offsets, k=500, exclude_seen=True, slack=16):
        """``fold_in`` of the documents, then ``recommend``'s candidates, scores and order per document: (rec_ids, rec_scores,
        rec_lengths), what ``evaluate.ranking_metrics`` takes.  The (context, context_offsets) of
        ``evaluate.split_holdout`` go in as they are."""
        factors, key, offsets = self._fold_in(indices, doc_offsets, None)
        with torch.cuda.device(self.device):
            upos = torch.arange(factors.shape[0], dtype=torch.int64, device=self.device)
            return _recommend_rows(factors, None, upos, self.item_factors, self.items, k, slack,
                                   offsets if exclude_seen else None, key, lambda q: "document %d" % q, "holds",
                                   "exclude_seen")


# ---- Bayesian Personalised Ranking --------------------------------------------------------------------------------------
OPTIMIZERS = ("adagrad", "sgd")
ADAGRAD_INIT = 0.1           # optax.adagrad's initial accumulator value, as everywhere in this package
FIT_GROUP = 64               # steps per sampler launch of BPR.fit


def _step_means(sums, counts):
    """Per step the fp64 sum divided by its count on the host; NaN for a step that counted nothing."""
    return [float(s) / int(n) if n else float("nan") for s, n in zip(sums, counts)]


class _SampledSGD(_Factorization):
    """What the models trained by sampled SGD through the row-sparse engine share (``BPR`` and its subclasses, ``SGNS``):
    the hyper-parameters, the seeded tables with their Adagrad accumulators, the update, the tail of ``train_steps`` and
    ``fit``.  A subclass provides ``sample`` and ``train_steps``."""

    def _configure(self, user, item, rank, reg, lr, optimizer, batch, seed, init_scale, device):
        """The checks that need no device, then the hyper-parameters as attributes; returns the flat (user, item) tensors."""
        rank = int(rank)
        _, top, mult = ops.bpr_geometry()
        if not mult <= rank <= top or rank % mult:
            raise ValueError("rank = %d is not a multiple of %d in [%d, %d]" % (rank, mult, mult, top))
        reg, lr = float(reg), float(lr)
        f32_max = float(np.finfo(np.float32).max)
        if not (math.isfinite(reg) and 0.0 <= reg <= f32_max):
            raise ValueError("reg = %r must be finite (as a float32) and not negative" % (reg,))
        if not (math.isfinite(lr) and abs(lr) <= f32_max):
            raise ValueError("lr = %r must be finite (as a float32)" % (lr,))
        if optimizer not in OPTIMIZERS:
            raise ValueError("optimizer must be 'adagrad' or 'sgd', got %r" % (optimizer,))
        batch = int(batch)
        if not 1 <= batch <= 2 ** 31 - 1:
            raise ValueError("batch = %d outside [1, 2^31 - 1]" % batch)
        user, item = _tensor(user, "user"), _tensor(item, "item")
        _same_length("user and item", user, item)
        if user.numel() == 0:
            raise ValueError("no (user, item) pair: BPR needs at least one seen pair")
        self._set_device(user, item, device)
        self.rank, self.reg, self.lr, self.optimizer, self.batch, self.seed = rank, reg, lr, optimizer, batch, int(seed)
        self.init_scale = float(rank) ** -0.5 if init_scale is None else float(init_scale)
        self.step = 0
        return user, item

    def _new_tables(self, *rows):
        """(a table [n, rank] per entry of `rows`, then their Adagrad accumulators): ``randn * init_scale`` from the seeded
        CPU generator in the order given (users first)."""
        dev, rank = self.device, self.rank
        gen = torch.Generator(device="cpu").manual_seed(self.seed)
        tables = [(torch.randn(n, rank, generator=gen) * self.init_scale).to(dev).contiguous() for n in rows]
        return tuple(tables) + tuple(torch.full((n, rank), ADAGRAD_INIT, dtype=torch.float32, device=dev) for n in rows)

    def _stream(self, seed, step0):
        """(seed, first step) of a ``sample`` call: the model's seed and the next step to take where None."""
        return self.seed if seed is None else int(seed), self.step if step0 is None else int(step0)

    def _apply(self, tables, accums, ids, bounds, grads, table_of=None):
        """One update of the tables (rows [bounds[n], bounds[n + 1]) of the stacked row space) through the row-sparse engine:
        id tensor k indexes table ``table_of[k]`` (ascending; by default ``ids[0]`` the first table and the others the
        second), `grads` holds one row per id in that order.  Adagrad sorts and updates all tables at once, SGD one table
        after the other; no id, no launch."""
        table_of = [0] + [1] * (len(ids) - 1) if table_of is None else table_of
        if self.optimizer == "adagrad":
            if grads.shape[0]:
                sorted_ids, perm = ops.segment_sort_multi(ids, [bounds[n] for n in table_of], bounds[-1])
                ops.sparse_adagrad_multi(tables, accums, bounds, sorted_ids, perm, grads, self.lr)
            return
        at = 0
        for n, table in enumerate(tables):
            own = [t for t, owner in zip(ids, table_of) if owner == n]
            count = sum(t.numel() for t in own)
            if count:
                own = own[0] if len(own) == 1 else ops.concat_offset_ids(own, [0] * len(own))
                sorted_ids, perm = ops.segment_sort(own, bounds[n + 1] - bounds[n])
                ops.sparse_sgd(table, sorted_ids, perm, grads[at:at + count], self.lr)
            at += count

    def _run_steps(self, K, what, one_step, rows=1):
        """The tail every ``train_steps`` shares: the failure word zeroed, ``one_step(k)`` = the `rows` fp64 device scalars
        of step k for k < K, ``step += K``, the word read (`what` words its refusal).  Returns float64[rows, K] on the host."""
        self._failed.zero_()
        sums = torch.empty((rows, K), dtype=torch.float64, device=self.device)
        for k in range(K):
            for r, value in enumerate(one_step(k)):
                sums[r, k] = value
        self.step += K
        self._raise_bad_position(what)
        return sums.cpu().numpy()

    @staticmethod
    def _check_K(K):
        K = int(K)
        if K < 1:
            raise ValueError("K = %d below 1" % K)
        return K

    def fit(self, steps):
        """`steps` steps in groups of 64 (one sampler launch per group); returns every step's mean loss."""
        losses, steps = [], int(steps)
        for a in range(0, steps, FIT_GROUP):
            losses += self.train_steps(min(FIT_GROUP, steps - a))
        return losses

    @staticmethod
    def _ordered_share(d, mask):
        """The share of the differences `d` under `mask` that are positive, a tie counting half; NaN under an empty mask."""
        n = int(mask.sum())
        wins, ties = int(((d > 0) & mask).sum()), int(((d == 0) & mask).sum())
        return (wins + 0.5 * ties) / n if n else float("nan")


class BPR(_SampledSGD):
    """Matrix factorisation trained on the ranking itself (Rendle, Freudenthaler, Gantner, Schmidt-Thieme, UAI 2009).

        model = BPR.from_documents(indices, doc_offsets, rank=64)       # user = document, a repeated id is one seen pair
        losses = model.fit(steps=2000)                                  # the mean loss of every step
        rec_ids, rec_scores, rec_lengths = model.recommend(users, k=500)     # straight into evaluate.ranking_metrics

    Step.  ``batch`` triples (user u, seen item i, unseen item j) are drawn on the device (``ops.bpr_sample``: Philox keyed
    by ``seed``, a function of (seed, step, slot) and the seen pairs alone; a triple whose 15 candidates were all seen is
    dropped: ``valid = 0``).  The objective of a step is the sum over its valid triples of ``softplus(-d) + (reg / 2)
    (|x_u|^2 + |y_i|^2 + |y_j|^2)``, ``d = x_u . y_i - x_u . y_j``.  ``ops.bpr_fwd_bwd`` writes one gradient row per
    occurrence; rows of a repeated id add (the engine's segment sum in a fixed order: Rendle's per-triple SGD taken as a
    minibatch) and the row-sparse engine applies Adagrad (``ops.sparse_adagrad_multi`` over both tables at once) or SGD
    (``ops.sparse_sgd``, users then items).  The fit is a function of the inputs and the seed.

    ``users`` / ``items``: int32 ascending ids; ``user_factors`` / ``item_factors``: float32 [nu, rank] / [ni, rank], both
    ``randn * init_scale`` from the seeded CPU generator (users first); ``step``: the steps taken so far."""

    def __init__(self, user, item, rank=64, reg=0.01, lr=0.05, optimizer="adagrad", batch=65536, seed=0, init_scale=None,
                 device=None):
        user, item = self._configure(user, item, rank, reg, lr, optimizer, batch, seed, init_scale, device)
        with torch.cuda.device(self.device):
            nu, ni = self._index_seen(user, item)
            self._init_tables(nu, ni)

    def _index_seen(self, user, item):
        """users / items, the CSR of the seen pairs on the host and on the device; returns (nu, ni)."""
        _, upos, ipos = self._index_pairs(user, item)
        return self._set_seen(upos, ipos)

    def _set_seen(self, upos, ipos):
        """The CSR of the seen pairs of the events (upos, ipos) on the host and on the device; returns (nu, ni)."""
        nu = int(self.users.numel())
        key = torch.unique((upos << 32) | ipos)                     # repeated events collapse to one seen pair
        self._set_pairs(key, _host_offsets(torch.bincount(key >> 32, minlength=nu)))
        self._offsets_dev = torch.from_numpy(self._user_offsets).to(self.device)    # the sampler reads the CSR on the device
        return nu, int(self.items.numel())

    def _init_tables(self, nu, ni):
        self.user_factors, self.item_factors, self.user_accum, self.item_accum = self._new_tables(nu, ni)

    nnz = property(lambda self: int(self._key.numel()))

    # ---- training -------------------------------------------------------------------------------------------------------
    def sample(self, K, step0=None, seed=None):
        """(u, i, j, valid) int32 [K, batch] and dropped int32[K]: the triples of the global steps step0 .. step0 + K - 1
        (``step0`` = the next step to take when None) as positions into ``users`` / ``items``."""
        with torch.cuda.device(self.device):
            return ops.bpr_sample(self._offsets_dev, self._row_upos, self._row_ipos, self.users.numel(), self.items.numel(),
                                  *self._stream(seed, step0), int(K), self.batch)

    def _update(self, u, i, j, grads):
        nu, ni = int(self.users.numel()), int(self.items.numel())
        self._apply([self.user_factors, self.item_factors], [self.user_accum, self.item_accum], [u, i, j], [0, nu, nu + ni],
                    grads)

    def train_steps(self, K):
        """K steps: one sampler launch, then per step the forward / backward, the sort and the update.  Returns the mean
        loss over the valid triples of every step (an fp64 sum of the per-triple losses divided on the host; NaN for a step
        without a valid triple).  Raises ``FactorizationError`` when a kernel met a position outside its table."""
        K = self._check_K(K)
        with torch.cuda.device(self.device):
            u, i, j, valid, dropped = self.sample(K)

            def one_step(k):
                loss_t, _, grads = ops.bpr_fwd_bwd(self.user_factors, self.item_factors, u[k], i[k], j[k], valid[k], self.reg,
                                                   failed=self._failed)
                self._update(u[k], i[k], j[k], grads)
                return (loss_t.to(torch.float64).sum(),)
            sums = self._run_steps(K, "a BPR step met a position outside its table (bit 30)", one_step)
            return _step_means(sums[0], self.batch - dropped.cpu().numpy().astype(np.int64))

    def auc(self, K=1, seed=None):
        """The fraction of K * batch sampled triples (valid ones) that the model orders correctly, ``d > 0``; a tie counts
        half.  The triples are steps 0 .. K - 1 of `seed` (``self.seed + 1`` when None: not a training stream, and the same
        triples before and after training).  NaN when no triple is valid."""
        with torch.cuda.device(self.device):
            u, i, j, valid, _ = self.sample(int(K), step0=0, seed=self.seed + 1 if seed is None else seed)
            self._failed.zero_()
            _, d, _ = ops.bpr_fwd_bwd(self.user_factors, self.item_factors, u.reshape(-1), i.reshape(-1), j.reshape(-1),
                                      valid.reshape(-1), self.reg, want_grads=False, want_diff=True, failed=self._failed)
            self._raise_bad_position("auc met a position outside its table (bit 30)")
            return self._ordered_share(d, valid.reshape(-1) != 0)


# ---- WARP ---------------------------------------------------------------------------------------------------------------
RANK_WEIGHTS = ("harmonic", "log1p")


def warp_rank_weight(rank_weight, ni):
    """float32[ni + 1] on the host: entry r is the step weight of an estimated rank r.  "harmonic": H_r = sum_{k <= r} 1 / k
    (WSABIE's), an fp64 cumulative sum rounded once, entry 0 = 0; "log1p": ln(1 + r); or an array of ni + 1 finite,
    non-negative values taken as they are."""
    ni = int(ni)
    if isinstance(rank_weight, str):
        if rank_weight not in RANK_WEIGHTS:
            raise ValueError("rank_weight must be 'harmonic', 'log1p' or an array of ni + 1 values, got %r" % (rank_weight,))
        r = np.arange(ni + 1, dtype=np.float64)
        if rank_weight == "harmonic":
            table = np.concatenate([[0.0], np.cumsum(1.0 / r[1:])])
        else:
            table = np.log1p(r)
        return table.astype(np.float32)
    table = np.asarray(rank_weight.detach().cpu().numpy() if isinstance(rank_weight, torch.Tensor) else rank_weight, np.float64)
    if table.shape != (ni + 1,):
        raise ValueError("rank_weight holds %s values, not ni + 1 = %d" % (table.shape, ni + 1))
    if not np.isfinite(table).all() or (table < 0).any() or (table > float(np.finfo(np.float32).max)).any():
        raise ValueError("rank_weight must hold finite (as float32), non-negative values")
    return table.astype(np.float32)


class WARP(BPR):
    """Matrix factorisation trained by WARP, the weighted approximate-rank pairwise loss (Weston, Bengio, Usunier, "WSABIE",
    IJCAI 2011): BPR's model, state and update, with the negative searched for instead of drawn.

        model = WARP.from_documents(indices, doc_offsets, rank=64, max_trials=32)
        losses = model.fit(steps=2000)                      # model.mean_trials: how hard negatives have become, per step
        rec_ids, rec_scores, rec_lengths = model.recommend(users, k=500)

    Step.  Per slot a seen pair (u, i) and up to ``max_trials`` candidates come from BPR's Philox stream; the first unseen
    candidate j with ``x_u . y_i - x_u . y_j < margin`` is the negative; with N unseen candidates walked the positive's rank
    is estimated as ``r = max(1, (ni - len_u) // N)`` and the slot's objective is ``rank_weight[r] * (margin - d) + (reg / 2)
    (|x_u|^2 + |y_i|^2 + |y_j|^2)``.  A slot whose candidates all keep the margin is dropped (``valid = 0``).  One
    ``ops.warp_step`` call does all of it (esr_warp.hip; the rule is esr_warp_sample.h's); the update is ``BPR``'s.

    The constructor arguments, ``users`` / ``items``, the factors, the accumulators and ``step`` are ``BPR``'s; ``auc``
    (over BPR's uniformly drawn triples), ``score`` and ``recommend`` are inherited."""

    def __init__(self, user, item, rank=64, reg=0.01, lr=0.05, optimizer="adagrad", batch=65536, seed=0, init_scale=None,
                 device=None, max_trials=32, margin=1.0, rank_weight="harmonic"):
        top, _, _ = ops.warp_geometry()
        max_trials, margin = int(max_trials), float(margin)
        if not 1 <= max_trials <= top:
            raise ValueError("max_trials = %d outside [1, %d]" % (max_trials, top))
        if not (math.isfinite(margin) and abs(margin) <= float(np.finfo(np.float32).max)):
            raise ValueError("margin = %r must be finite (as a float32)" % (margin,))
        if isinstance(rank_weight, str) and rank_weight not in RANK_WEIGHTS:
            raise ValueError("rank_weight must be 'harmonic', 'log1p' or an array of ni + 1 values, got %r" % (rank_weight,))
        super().__init__(user, item, rank=rank, reg=reg, lr=lr, optimizer=optimizer, batch=batch, seed=seed,
                         init_scale=init_scale, device=device)
        self.max_trials, self.margin = max_trials, margin
        self.rank_weight = torch.from_numpy(warp_rank_weight(rank_weight, self.items.numel())).to(self.device)
        self.mean_trials = []

    def _warp_step(self, step, want_grads):
        return ops.warp_step(self.user_factors, self.item_factors, self._offsets_dev, self._row_upos, self._row_ipos,
                             self.rank_weight, self.seed, step, self.batch, self.max_trials, self.margin, self.reg,
                             want_grads=want_grads, failed=self._failed)

    def step_triples(self, step=None):
        """(u, i, j, valid, trials) int32[batch] of global step `step` (the next step to take when None) against the
        factors as they stand: forward only, nothing is updated."""
        with torch.cuda.device(self.device):
            self._failed.zero_()
            out = self._warp_step(self.step if step is None else int(step), False)
            self._raise_bad_position("a WARP step met a position outside its table (bit 30)")
        return out[:5]

    def train_steps(self, K):
        """K steps: per step one ``ops.warp_step`` call, the sort and the update.  Returns the mean loss over the valid slots
        of every step (an fp64 sum of the per-slot losses divided on the host; NaN for a step without a valid slot) and
        appends every step's mean ``trials`` to ``mean_trials``.  Raises ``FactorizationError`` when the kernel met a
        position outside its table."""
        K = self._check_K(K)
        with torch.cuda.device(self.device):
            step0 = self.step

            def one_step(k):
                u, i, j, valid, trials, loss_t, _, grads = self._warp_step(step0 + k, True)
                self._update(u, i, j, grads)
                return loss_t.to(torch.float64).sum(), valid.sum(), trials.sum()
            sums = self._run_steps(K, "a WARP step met a position outside its table (bit 30)", one_step, rows=3)
        self.mean_trials += [float(n) / self.batch for n in sums[2]]
        return _step_means(sums[0], sums[1])


# ---- hybrid BPR: entities as sums of feature embeddings -----------------------------------------------------------------
def _feature_coo(features, side):
    """(entity int64, feature int64, weight float32 or None) of a ``(entity_id, feature_id, weight or None)`` triple as flat
    host arrays, with the refusals that need nothing else: lengths, integer ids, finite weights."""
    if len(features) != 3:
        raise ValueError("%s_features must be (entity_id, feature_id, weight or None)" % side)
    ent, feat = _tensor(features[0], "entity_id"), _tensor(features[1], "feature_id")
    _same_length("%s_features' entity_id and feature_id" % side, ent, feat)
    if ent.dtype.is_floating_point or feat.dtype.is_floating_point or ent.dtype == torch.bool or feat.dtype == torch.bool:
        raise TypeError("%s_features' entity_id and feature_id must be integer arrays" % side)
    ent, feat = ent.cpu().numpy().astype(np.int64), feat.cpu().numpy().astype(np.int64)
    weight = None
    if features[2] is not None:
        w = _tensor(features[2], "weight")
        _same_length("%s_features' entity_id and weight" % side, _tensor(features[0], "entity_id"), w)
        w = w.cpu().numpy().astype(np.float64)
        if not np.isfinite(w).all() or (np.abs(w) > float(np.finfo(np.float32).max)).any():
            raise ValueError("%s_features: a weight is not finite (as a float32)" % side)
        weight = w.astype(np.float32)
    return ent, feat, weight


def _bag_table(epos, fpos, weight, n, identity, side):
    """The bag table of n entities on the host: (offsets int64[n + 1], feat int32[nnz], weight float32[nnz] or None).  With
    `identity` entity e's bag starts with the indicator row e (weight 1) and the side features' rows follow, shifted by n;
    within a bag the side features ascend.  A repeated (entity, feature) pair is refused."""
    key = (epos << 32) | fpos
    order = np.argsort(key, kind="stable")
    key = key[order]
    if key.size > 1 and (key[1:] == key[:-1]).any():
        at = int(np.flatnonzero(key[1:] == key[:-1])[0])
        raise ValueError("%s_features: the pair (entity position %d, feature position %d) is given twice"
                         % (side, key[at] >> 32, key[at] & 0xFFFFFFFF))
    lead = 1 if identity else 0
    counts = np.bincount(epos, minlength=n).astype(np.int64)
    offsets = _host_offsets(counts + lead)
    nnz = int(offsets[-1])
    if nnz < 1:
        raise ValueError("%s side: no entity has a feature" % side)
    if nnz > 2 ** 31 - 1:
        raise ValueError("%s side: %d feature occurrences exceed 2^31 - 1" % (side, nnz))
    e_sorted = key >> 32
    starts = _host_offsets(counts)[:-1]
    at = offsets[e_sorted] + lead + (np.arange(key.size) - starts[e_sorted])
    feat = np.empty(nnz, np.int32)
    feat[at] = (key & 0xFFFFFFFF) + (n if identity else 0)
    w = None
    if weight is not None:
        w = np.ones(nnz, np.float32)
        w[at] = weight[order]
    if identity:
        feat[offsets[:-1]] = np.arange(n, dtype=np.int32)
    return offsets, feat, w


class _Bags:
    """A bag table on the device (``ops.bag_sum`` / ``ops.bag_expand``) and its bags' lengths."""

    def __init__(self, offsets, feat, weight, dev):
        self.n = offsets.size - 1
        self.offsets = torch.from_numpy(offsets).to(dev)
        self.feat = torch.from_numpy(feat).to(dev)
        self.weight = None if weight is None else torch.from_numpy(weight).to(dev)
        self.lengths = torch.from_numpy(np.diff(offsets)).to(dev)

    def args(self):
        return self.offsets, self.feat, self.weight


class HybridBPR(BPR):
    """BPR over users and items that are weighted sums of feature embeddings (Kula, "Metadata Embeddings for User and Item
    Cold-start Recommendations", 2015: LightFM's model, trained with the BPR step).

        model = HybridBPR(user, item, item_features=(item_id, tag_id, None), rank=64)
        losses = model.fit(steps=2000)
        new_ids, new_rows = model.compose_items(new_item_id, new_tag_id)      # items that were in no training pair
        rec_ids, rec_scores, rec_lengths = model.recommend(users, k=500, extra_items=(new_ids, new_rows))

    Representation.  ``x_u = sum_f w[u, f] e_f`` over the features of u's bag (``ops.bag_sum``: a fmaf chain in the bag's
    order), and the same for items.  ``*_features`` is ``(entity_id, feature_id, weight or None)`` in COO form; raw ids
    become positions through ``torch.unique`` / a sorted search.  ``identity[side]`` gives every entity one indicator
    feature of weight 1, placed first in its bag; its rows are rows [0, n) of the side's embedding table and the side
    features' rows follow in ascending id (``user_feature_ids`` / ``item_feature_ids``).  With identity-only bags the model
    is BPR's.

    Step.  Compose the batch's rows (``P`` for u, ``Q`` for [i ; j]), run ``ops.bpr_fwd_bwd`` on them with reg = 0, hand the
    gradient rows back to the features with ``ops.bag_expand`` (which adds ``reg * e_f`` per occurrence) and update the
    embedding tables through the row-sparse engine as BPR does.  The objective of a step is ``sum_valid softplus(-d) +
    (reg / 2) sum |e_f|^2`` over every feature occurrence of the valid triples' three bags.

    ``user_embeddings`` [nfu, rank] / ``item_embeddings`` [nfi, rank] are initialised like BPR's tables (seeded CPU
    generator, users first); ``user_factors`` / ``item_factors`` are the composed tables of every known entity
    (``user_rows()`` / ``item_rows()``), which ``score``, ``recommend`` and ``auc`` read."""

    def __init__(self, user, item, user_features=None, item_features=None, identity=(True, True), rank=64, reg=0.01, lr=0.05,
                 optimizer="adagrad", batch=65536, seed=0, init_scale=None, device=None):
        identity = tuple(bool(v) for v in identity)
        if len(identity) != 2:
            raise ValueError("identity must be a (user side, item side) pair")
        given = (user_features, item_features)
        for side, feats, ident in zip(("user", "item"), given, identity):
            if feats is None and not ident:
                raise ValueError("%s side: identity is off and no %s_features are given: its entities would have no feature"
                                 % (side, side))
        coo = [None if f is None else _feature_coo(f, side) for side, f in zip(("user", "item"), given)]
        # (the pairs' own host checks come first, as BPR's; the features are then checked against the pairs' ids on the host)
        ids = [_tensor(user, "user"), _tensor(item, "item")]
        tables = []
        if not any(t.dtype.is_floating_point for t in ids) and ids[0].numel() == ids[1].numel() and ids[0].numel():
            for side, t, c, ident in zip(("user", "item"), ids, coo, identity):
                tables.append(self._host_bags(side, np.unique(t.cpu().numpy().astype(np.int64)), c, ident))
        user, item = self._configure(user, item, rank, reg, lr, optimizer, batch, seed, init_scale, device)
        self.identity = identity
        with torch.cuda.device(self.device):
            nu, ni = self._index_seen(user, item)
            (ubag, ufeat), (ibag, ifeat) = tables
            self._user_bags, self._item_bags = _Bags(*ubag, self.device), _Bags(*ibag, self.device)
            self.user_feature_ids = torch.from_numpy(ufeat).to(self.device)
            self.item_feature_ids = torch.from_numpy(ifeat).to(self.device)
            self._init_tables((nu if identity[0] else 0) + ufeat.size, (ni if identity[1] else 0) + ifeat.size)

    @staticmethod
    def _host_bags(side, known, coo, identity):
        """((offsets, feat, weight), side feature ids int64 ascending) of one side on the host; `known` = the side's entity
        ids, ascending."""
        n = known.size
        if coo is None:
            ent = fpos = np.zeros(0, np.int64)
            weight, feature_ids = None, np.zeros(0, np.int64)
        else:
            ent, feat, weight = coo
            at = np.searchsorted(known, ent).clip(max=n - 1)
            if ent.size and (known[at] != ent).any():
                raise ValueError("%s_features: entity id %d occurs in no (user, item) pair"
                                 % (side, int(ent[known[at] != ent][0])))
            ent = at.astype(np.int64)
            feature_ids, fpos = np.unique(feat, return_inverse=True)
            fpos = fpos.reshape(-1).astype(np.int64)
            if n + feature_ids.size > 2 ** 31 - 1:
                raise ValueError("%s side: more than 2^31 - 1 feature rows" % side)
        return _bag_table(ent, fpos, weight, n, identity, side), feature_ids

    def _init_tables(self, nfu, nfi):
        self.user_embeddings, self.item_embeddings, self.user_accum, self.item_accum = self._new_tables(nfu, nfi)
        self._composed = None

    # ---- the composed tables ------------------------------------------------------------------------------------------------
    def _compose_all(self):
        key = (self.step, self.user_embeddings._version, self.item_embeddings._version)
        if self._composed is None or self._composed[0] != key:
            with torch.cuda.device(self.device):
                self._failed.zero_()
                rows = (ops.bag_sum(self.user_embeddings, *self._user_bags.args(), failed=self._failed),
                        ops.bag_sum(self.item_embeddings, *self._item_bags.args(), failed=self._failed))
                self._raise_bad_position("a bag names a feature position outside its table (bit 30)")
            self._composed = (key,) + rows
        return self._composed[1:]

    def user_rows(self):
        """float32[nu, rank]: every known user composed from the embeddings as they stand (kept until the next step)."""
        return self._compose_all()[0]

    def item_rows(self):
        """float32[ni, rank]: every known item composed from the embeddings as they stand (kept until the next step)."""
        return self._compose_all()[1]

    user_factors = property(user_rows)
    item_factors = property(item_rows)

    # ---- training -------------------------------------------------------------------------------------------------------
    def _step(self, u, ij, valid, valid2, oo_u, oo_i, Mu, Mi, ar, ar_b):
        """One step on the triples (u, [i ; j]); returns loss_t."""
        B = u.numel()
        ue, ie, ub, ib = self.user_embeddings, self.item_embeddings, self._user_bags, self._item_bags
        P = ops.bag_sum(ue, *ub.args(), rows=u, failed=self._failed)
        Q = ops.bag_sum(ie, *ib.args(), rows=ij, failed=self._failed)
        loss_t, _, grads = ops.bpr_fwd_bwd(P, Q, ar, ar, ar_b, valid, 0.0, failed=self._failed)
        out_feat = torch.empty(Mu + Mi, dtype=torch.int32, device=self.device)
        out_grads = torch.empty((Mu + Mi, self.rank), dtype=torch.float32, device=self.device)
        fu, fi, gu, gi = out_feat[:Mu], out_feat[Mu:], out_grads[:Mu], out_grads[Mu:]
        ops.bag_expand(ue, *ub.args(), u, grads[:B], valid, oo_u, Mu, self.reg, out=(fu, gu), failed=self._failed)
        ops.bag_expand(ie, *ib.args(), ij, grads[B:], valid2, oo_i, Mi, self.reg, out=(fi, gi), failed=self._failed)
        nfu, nfi = ue.shape[0], ie.shape[0]
        self._apply([ue, ie], [self.user_accum, self.item_accum], [fu, fi], [0, nfu, nfu + nfi], out_grads)
        return loss_t

    def train_steps(self, K):
        """K steps: one sampler launch, every step's ``out_offsets`` by one torch scan, one read of the expanded sizes, then
        per step the two compositions, the forward / backward, the two expansions, the sort and the update.  Returns
        BPR's per-step mean loss.  Raises ``ValueError`` when a step's expanded occurrences exceed 2^31 - 1 and
        ``FactorizationError`` when a kernel met a position outside its table."""
        K = self._check_K(K)
        dev, B = self.device, self.batch
        with torch.cuda.device(dev):
            u, i, j, valid, dropped = self.sample(K)
            ij, valid2 = torch.cat([i, j], dim=1), torch.cat([valid, valid], dim=1)
            oo_u = torch.zeros((K, B + 1), dtype=torch.int64, device=dev)
            oo_i = torch.zeros((K, 2 * B + 1), dtype=torch.int64, device=dev)
            oo_u[:, 1:] = torch.cumsum(self._user_bags.lengths[u.to(torch.int64)], 1)
            oo_i[:, 1:] = torch.cumsum(self._item_bags.lengths[ij.to(torch.int64)], 1)
            sizes = torch.stack([oo_u[:, -1], oo_i[:, -1]]).cpu().numpy()            # the one read of sizes
            if int((sizes[0] + sizes[1]).max()) > 2 ** 31 - 1:
                raise ValueError("a step expands to %d feature occurrences, above 2^31 - 1: lower batch"
                                 % int((sizes[0] + sizes[1]).max()))
            ar = torch.arange(2 * B, dtype=torch.int32, device=dev)

            def one_step(k):
                loss_t = self._step(u[k], ij[k], valid[k], valid2[k], oo_u[k], oo_i[k], int(sizes[0, k]), int(sizes[1, k]),
                                    ar[:B], ar[B:])
                return (loss_t.to(torch.float64).sum(),)
            sums = self._run_steps(K, "a hybrid BPR step met a position outside its table (bit 30)", one_step)
            self._composed = None
            return _step_means(sums[0], self.batch - dropped.cpu().numpy().astype(np.int64))

    # ---- cold start -------------------------------------------------------------------------------------------------------
    def _compose_new(self, side, entity_id, feature_id, weight):
        known = (self.users if side == "user" else self.items).cpu().numpy().astype(np.int64)
        feature_ids = (self.user_feature_ids if side == "user" else self.item_feature_ids).cpu().numpy()
        table = self.user_embeddings if side == "user" else self.item_embeddings
        ent, feat, weight = _feature_coo((entity_id, feature_id, weight), side)
        if ent.size == 0:
            raise ValueError("compose_%ss: no (entity, feature) pair" % side)
        if ent.min() < 0 or ent.max() >= 2 ** 31 - 1:
            raise ValueError("entity ids must lie in [0, 2^31 - 1)")
        if np.isin(ent, known).any():
            raise ValueError("compose_%ss: %s %d was in training: recommend ranks it already"
                             % (side, side, int(ent[np.isin(ent, known)][0])))
        fpos = np.searchsorted(feature_ids, feat).clip(max=max(feature_ids.size - 1, 0))
        if feature_ids.size == 0 or (feature_ids[fpos] != feat).any():
            bad = feat if feature_ids.size == 0 else feat[feature_ids[fpos] != feat]
            raise ValueError("compose_%ss: feature id %d was not seen in training" % (side, int(bad[0])))
        ids, epos = np.unique(ent, return_inverse=True)
        shift = known.size if self.identity[0 if side == "user" else 1] else 0
        offsets, bag_feat, w = _bag_table(epos.reshape(-1).astype(np.int64), fpos.astype(np.int64) + shift, weight, ids.size,
                                          False, side)
        with torch.cuda.device(self.device):
            bags = _Bags(offsets, bag_feat, w, self.device)
            self._failed.zero_()
            rows = ops.bag_sum(table, *bags.args(), failed=self._failed)
            self._raise_bad_position("compose_%ss met a feature position outside the table (bit 30)" % side)
            return torch.from_numpy(ids.astype(np.int32)).to(self.device), rows

    def compose_items(self, entity_id, feature_id, weight=None):
        """(ids int32[n] ascending, rows float32[n, rank]) of items that were NOT in training, composed from known features
        only (no identity row).  A feature id the model never saw, a known item or a repeated pair raises ``ValueError``."""
        return self._compose_new("item", entity_id, feature_id, weight)

    def compose_users(self, entity_id, feature_id, weight=None):
        """``compose_items`` for users: rows to score against ``item_rows()`` (``ops.retrieve_topk``, ``ops.als_predict``)."""
        return self._compose_new("user", entity_id, feature_id, weight)

    def recommend(self, users, k=500, exclude_seen=True, slack=16, extra_items=None):
        """``BPR.recommend`` on the composed tables.  ``extra_items`` = the ``(ids, rows)`` of ``compose_items``: those items
        are ranked together with the known ones by the same (score descending, item id ascending) order and are never
        "seen"."""
        if extra_items is None:
            return self._recommend(users, k, slack, exclude_seen)
        with torch.cuda.device(self.device):
            upos = self._positions(users, self.users).to(torch.int64)
            rows, items, key = self.item_factors, self.items, self._key
            ids, extra = extra_items
            ids = _tensor(ids, "extra ids").to(self.device).to(torch.int64)
            if not isinstance(extra, torch.Tensor) or extra.dtype != torch.float32 or extra.dim() != 2 or \
                    tuple(extra.shape) != (ids.numel(), self.rank):
                raise ValueError("extra_items must be (ids[n], float32 rows[n, rank])")
            both = torch.cat([items.to(torch.int64), ids])
            if torch.unique(both).numel() != both.numel():
                raise ValueError("extra_items repeats an item id or names a known item")
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= 2 ** 31 - 1):
                raise ValueError("item ids must lie in [0, 2^31 - 1)")
            order = torch.argsort(both)
            place = torch.empty_like(order)
            place[order] = torch.arange(order.numel(), device=self.device)      # old position -> position by id
            rows = torch.cat([rows, extra.to(self.device)])[order].contiguous()
            items = both[order].to(torch.int32).contiguous()
            key = ((key >> 32) << 32) | place[key & 0xFFFFFFFF]                 # (monotone per user: still ascending)
            return _recommend_rows(self.user_factors, None, upos, rows, items, k, slack,
                                   self._user_offsets if exclude_seen else None, key,
                                   lambda q: "user %d" % int(_tensor(users, "users")[q]), "has seen", "exclude_seen")


# ---- sequential recommendation: the factorised personalised Markov chain -------------------------------------------------
def _tail_bags(ipos, offsets, window, dev):
    """The bag table (``_Bags``) whose bag d is the last ``c = min(length, window)`` entries of row d of the CSR (ipos int64
    on the device, host offsets), oldest first, every weight ``float32(1) / float32(c)``; None when no row has an entry."""
    lens = np.diff(offsets)
    c = np.minimum(lens, window)
    bag_offsets = _host_offsets(c)
    if int(bag_offsets[-1]) == 0:
        return None
    at = np.repeat(offsets[1:] - c - bag_offsets[:-1], c) + np.arange(int(bag_offsets[-1]), dtype=np.int64)
    weight = np.repeat(np.float32(1.0) / np.maximum(c, 1).astype(np.float32), c)
    feat = ipos[torch.from_numpy(at).to(dev)].to(torch.int32).cpu().numpy()
    return _Bags(bag_offsets, feat, weight, dev)


class _Sequences:
    """What the two models over id sequences (``FPMC``, ``SGNS``) share: the events as a CSR by sequence -- ``users`` names
    the sequences -- and the serving of sequences given at query time."""

    def _set_sequences(self, upos, ipos, time):
        """The CSR of the events by sequence on the host and the device (``_seq_offsets``, ``_seq_upos`` / ``_seq_ipos``):
        a sequence's events in the order given, or by (time, order given).  Returns ipos int64 in the CSR's order."""
        dev = self.device
        if upos.numel() > 2 ** 31 - 1:
            raise ValueError("%d events exceed 2^31 - 1" % upos.numel())
        order = torch.arange(upos.numel(), device=dev) if time is None else torch.sort(time.to(dev), stable=True).indices
        order = order[torch.sort(upos[order], stable=True).indices]
        self._seq_offsets = _host_offsets(torch.bincount(upos, minlength=int(self.users.numel())))
        self._seq_offsets_dev = torch.from_numpy(self._seq_offsets).to(dev)
        self._seq_upos = upos[order].to(torch.int32).contiguous()
        self._seq_ipos = ipos[order].to(torch.int32).contiguous()
        return ipos[order]

    n_events = property(lambda self: int(self._seq_ipos.numel()))

    def _known_sequences(self, indices, doc_offsets):
        """(docs, ipos int64 on the device, host offsets) of the given sequences ``indices[doc_offsets[d]:doc_offsets[d +
        1]]``, reduced to the ids the model knows (the others are skipped)."""
        ids, off = _ids_and_offsets(indices, doc_offsets, self.device)
        ndocs = off.size - 1
        docs = torch.from_numpy(np.repeat(np.arange(ndocs, dtype=np.int64), np.diff(off))).to(self.device)
        ipos = self._positions(ids, self.items).to(torch.int64)
        known = ipos >= 0
        docs, ipos = docs[known], ipos[known]
        return docs, ipos, _host_offsets(torch.bincount(docs, minlength=ndocs))

    def _bag_rows(self, table, bags, n, what):
        """float32[n, rank]: ``ops.bag_sum`` of every bag of `bags` (``_tail_bags``) over `table`; zeros without bags."""
        if bags is None:
            return torch.zeros((n, self.rank), dtype=torch.float32, device=self.device)
        self._failed.zero_()
        rows = ops.bag_sum(table, *bags.args(), failed=self._failed)
        self._raise_bad_position("a %s names an item position outside the table (bit 30)" % what)
        return rows

    def _recommend_sequences(self, queries, item_rows, docs, ipos, k, slack, exclude_seen):
        """``_recommend_rows`` of one query row per given sequence; `exclude_seen` leaves out the sequence's own items."""
        ndocs = int(queries.shape[0])
        key = torch.unique((docs << 32) | ipos)
        seen_offsets = _host_offsets(torch.bincount(key >> 32, minlength=ndocs)) if exclude_seen else None
        return _recommend_rows(queries, None, torch.arange(ndocs, dtype=torch.int64, device=self.device), item_rows,
                               self.items, k, slack, seen_offsets, key, lambda q: "sequence %d" % q, "holds", "exclude_seen")


class FPMC(_Sequences, BPR):
    """The Factorised Personalised Markov Chain (Rendle, Freudenthaler, Schmidt-Thieme, WWW 2010) trained with the BPR step:
    BPR's user-item term plus a factorised transition term from the items just consumed -- "what comes next".

        model = FPMC.from_documents(indices, doc_offsets, window=3, rank=32)      # a document is a sequence in order
        losses = model.fit(steps=2000)
        rec_ids, rec_scores, rec_lengths = model.recommend(users, k=10)           # after each user's training sequence
        rec_ids, rec_scores, rec_lengths = model.recommend_sequences(ids, offsets, k=10)      # sessions of unseen users

    Model.  Four tables of one rank: ``user_factors`` U [nu, rank], ``item_factors`` A [ni, rank] (the item as the user term
    sees it), ``next_factors`` Bn [ni, rank] (the item as a successor) and ``prev_factors`` P [ni, rank] (the item as a
    predecessor).  An event is place t of user u's sequence -- the events in the order given, or by a stable sort on
    (user, time) with `time`; repeats are kept.  Its context is the ``c = min(t, window)`` items just before it and
    ``m = sum_l P_l / c`` over them (``ops.bag_sum``'s chain, oldest first).  ``score(u, t, i) = U_u . A_i + m . Bn_i``.

    Step.  ``batch`` slots (event, unseen item j) are drawn on the device (``ops.fpmc_sample``: BPR's Philox stream and
    BPR's negatives against the user's seen set).  The objective of a step is the sum over its valid slots of
    ``softplus(-d) + (reg / 2)(|U_u|^2 + |A_i|^2 + |A_j|^2 + |Bn_i|^2 + |Bn_j|^2 + sum_ctx |P_l|^2)``,
    ``d = score(i) - score(j)``.  ``ops.fpmc_fwd_bwd`` writes one gradient row per occurrence and the row-sparse engine
    updates the four tables: Adagrad in one sort and one launch, SGD table by table.  The fit is a function of the inputs
    and the seed.

    Serving.  A query is the row ``[U_u ; m]`` and an item the row ``[A_i ; Bn_i]``, both 2 rank wide, so ``score``,
    ``recommend`` and ``diversify`` are the base class's on those rows (``query_rows`` / ``item_rows``): for a known user m
    is built from the tail of the training sequence, the prediction of the NEXT event.  They re-score by the ALS predict
    kernel, which takes rows of at most ``predict_max_rank()``: serving needs ``2 rank <= predict_max_rank()``.

    The tables are ``randn * init_scale`` from the seeded CPU generator in the order U, A, Bn, P; the other constructor
    arguments, ``users`` / ``items`` and ``step`` are ``BPR``'s."""

    def __init__(self, user, item, time=None, window=1, rank=64, reg=0.01, lr=0.05, optimizer="adagrad", batch=65536, seed=0,
                 init_scale=None, device=None):
        top, _, _ = ops.fpmc_geometry()
        window = int(window)
        if not 1 <= window <= top:
            raise ValueError("window = %d outside [1, %d]" % (window, top))
        user, item = self._configure(user, item, rank, reg, lr, optimizer, batch, seed, init_scale, device)
        if time is not None:
            time = _tensor(time, "time")
            _same_length("user, item and time", user, item, time)
        self.window = window
        dev = self.device
        with torch.cuda.device(dev):
            _, upos, ipos = self._index_pairs(user, item)
            nu, ni = self._set_seen(upos, ipos)
            if nu + 3 * ni > 2 ** 31 - 1:
                raise ValueError("nu + 3 ni = %d rows exceed 2^31 - 1 (the row space of the update)" % (nu + 3 * ni))
            self._tails = _tail_bags(self._set_sequences(upos, ipos, time), self._seq_offsets, window, dev)
            self._init_tables(nu, ni)

    def _init_tables(self, nu, ni):
        (self.user_factors, self.item_factors, self.next_factors, self.prev_factors, self.user_accum, self.item_accum,
         self.next_accum, self.prev_accum) = self._new_tables(nu, ni, ni, ni)
        self._served = None

    # ---- training -------------------------------------------------------------------------------------------------------
    def sample(self, K, step0=None, seed=None):
        """(u, e, c, i, j, valid) int32 [K, batch] and dropped int32[K]: the slots of the global steps step0 .. step0 + K - 1
        (``step0`` = the next step to take when None) -- u, i, j positions into ``users`` / ``items``, e the event's number
        in the sequence CSR and c its context length."""
        with torch.cuda.device(self.device):
            return ops.fpmc_sample(self._seq_offsets_dev, self._seq_upos, self._seq_ipos, self._offsets_dev, self._row_ipos,
                                   self.users.numel(), self.items.numel(), self.window, *self._stream(seed, step0), int(K),
                                   self.batch)

    def _tables(self):
        return [self.user_factors, self.item_factors, self.next_factors, self.prev_factors]

    def _update(self, u, ij, ctx_ids, grads):
        """The engine over the four tables: the id list [u ; i ; j ; i ; j ; ctx_ids] of the gradient rows as the four
        segments u, ij = [i ; j] (for A), ij again (for Bn) and ctx_ids (the sort takes at most four)."""
        nu, ni = int(self.users.numel()), int(self.items.numel())
        ids, table_of = [u, ij, ij], [0, 1, 2]
        if ctx_ids.numel():
            ids, table_of = ids + [ctx_ids], table_of + [3]
        self._apply(self._tables(), [self.user_accum, self.item_accum, self.next_accum, self.prev_accum], ids,
                    [0, nu, nu + ni, nu + 2 * ni, nu + 3 * ni], grads, table_of)

    def train_steps(self, K):
        """K steps: one sampler launch, one scan of c over [K, batch] and ONE host read of the K totals; then per step the
        forward / backward, the sort and the update over the four tables.  Returns BPR's per-step mean loss.  Raises
        ``FactorizationError`` when a kernel met a position outside its table."""
        K = self._check_K(K)
        dev, B = self.device, self.batch
        with torch.cuda.device(dev):
            u, e, c, i, j, valid, dropped = self.sample(K)
            oo = torch.zeros((K, B + 1), dtype=torch.int64, device=dev)
            oo[:, 1:] = torch.cumsum(c, 1)
            host = torch.stack([oo[:, -1], dropped.to(torch.int64)]).cpu().numpy()       # the one read: totals and dropped
            tables, ij = self._tables(), torch.cat([i, j], dim=1)

            def one_step(k):
                loss_t, _, grads, ctx_ids = ops.fpmc_fwd_bwd(*tables, self._seq_ipos, u[k], e[k], c[k], i[k], j[k], valid[k],
                                                             self.reg, ctx_offsets=oo[k], M=int(host[0, k]),
                                                             failed=self._failed)
                self._update(u[k], ij[k], ctx_ids, grads)
                return (loss_t.to(torch.float64).sum(),)
            sums = self._run_steps(K, "an FPMC step met a position outside its table (bit 30)", one_step)
            self._served = None
            return _step_means(sums[0], B - host[1])

    def auc(self, K=1, seed=None):
        """``BPR.auc`` over FPMC's own slots: the fraction of K * batch sampled (event, unseen item) slots whose next item
        the model scores above the unseen one."""
        with torch.cuda.device(self.device):
            u, e, c, i, j, valid, _ = (t.reshape(-1) for t in
                                       self.sample(int(K), step0=0, seed=self.seed + 1 if seed is None else seed)[:7])
            self._failed.zero_()
            _, d, _, _ = ops.fpmc_fwd_bwd(*self._tables(), self._seq_ipos, u, e, c, i, j, valid, self.reg, want_grads=False,
                                          want_diff=True, failed=self._failed)
            self._raise_bad_position("auc met a position outside its table (bit 30)")
            return self._ordered_share(d, valid != 0)

    # ---- serving --------------------------------------------------------------------------------------------------------
    def _rows(self):
        top = predict_max_rank()
        if 2 * self.rank > top:
            raise ValueError("rank = %d: score, recommend and diversify re-score rows of 2 rank by the ALS predict kernel, "
                             "which takes at most %d: serving needs rank <= %d" % (self.rank, top, top // 2))
        key = (self.step,) + tuple(t._version for t in self._tables())
        if self._served is None or self._served[0] != key:
            self._served = (key, self.query_rows(), self.item_rows())
        return self._served[1:]

    def query_rows(self, users=None):
        """float32[n, 2 rank]: the rows ``[U_u ; m_u]`` of `users` (every known user in ``users``' order when None), m_u
        the context of the event that would follow u's training sequence: its last ``min(length, window)`` items by
        ``ops.bag_sum`` with the weights ``float32(1 / c)``, the chain the step kernel walks.  An unknown user gets NaN."""
        with torch.cuda.device(self.device):
            m = self._bag_rows(self.prev_factors, self._tails, int(self.users.numel()), "context")
            rows = torch.cat([self.user_factors, m], 1)
            if users is None:
                return rows.contiguous()
            upos = self._positions(users, self.users).to(torch.int64)
            nan = torch.full((), float("nan"), device=self.device)
            return torch.where((upos >= 0)[:, None], rows[upos.clamp(min=0)], nan).contiguous()

    def item_rows(self):
        """float32[ni, 2 rank]: the rows ``[A_i ; Bn_i]`` of every item in ``items``' order."""
        return torch.cat([self.item_factors, self.next_factors], 1).contiguous()

    def recommend_sequences(self, indices, doc_offsets, k=500, users=None, exclude_seen=True, slack=16):
        """``recommend``'s lists for GIVEN sequences ``indices[doc_offsets[d]:doc_offsets[d + 1]]`` (ids in order): the query
        of sequence d is ``[U_u ; m]`` with m built from its last ``window`` items that the model knows (unknown ids are
        skipped) and u = ``users[d]``; with ``users=None``, or for a user the model does not know, the user half is zero:
        pure session-based recommendation by the transition term.  `exclude_seen` leaves out the sequence's own items.
        Returns (rec_ids, rec_scores, rec_lengths), what ``evaluate.ranking_metrics`` takes; with a known user's training
        sequence the lists are ``recommend``'s."""
        with torch.cuda.device(self.device):
            docs, ipos, offsets = self._known_sequences(indices, doc_offsets)
            ndocs = offsets.size - 1
            item_rows = self._rows()[1]
            m = self._bag_rows(self.prev_factors, _tail_bags(ipos, offsets, self.window, self.device), ndocs, "context")
            half = torch.zeros_like(m)
            if users is not None:
                upos = self._positions(users, self.users).to(torch.int64)
                if upos.numel() != ndocs:
                    raise ValueError("users must name one user per sequence")
                half = torch.where((upos >= 0)[:, None], self.user_factors[upos.clamp(min=0)], half)
            return self._recommend_sequences(torch.cat([half, m], 1).contiguous(), item_rows, docs, ipos, k, slack, exclude_seen)


# ---- skip-gram with negative sampling ------------------------------------------------------------------------------------
NOISE_COLUMN = 1 << 32       # the mass of one column of the alias table: a 32-bit Philox word


def sgns_noise_masses(counts, power=0.75):
    """int64[ni] on the host: ``count ** power`` quantised to integer masses that sum to ``ni * 2^32`` exactly.  An item
    that occurs gets a mass of at least 1, one that never occurs mass 0.  The float64 targets are floored; what the
    floors (and the lifts to 1) leave over is spread over the occurring items in descending mass, one unit at a time."""
    counts = np.asarray(counts)
    if counts.ndim != 1 or counts.size < 1 or counts.dtype.kind not in "iu" or bool((counts < 0).any()):
        raise ValueError("counts must be a non-empty array of non-negative integers")
    power = float(power)
    if not (math.isfinite(power) and power >= 0.0):
        raise ValueError("power = %r must be finite and not negative" % (power,))
    ni = counts.size
    occurs = counts > 0
    n_occ = int(occurs.sum())
    if n_occ == 0:
        raise ValueError("no item occurs: the noise distribution is empty")
    total = ni * NOISE_COLUMN
    f = np.where(occurs, np.maximum(counts, 1).astype(np.float64) ** power, 0.0)
    masses = np.where(occurs, np.maximum(np.floor(f / f.sum() * total), 1.0), 0.0).astype(np.int64)
    rest = total - int(masses.sum())
    order = np.argsort(-masses, kind="stable")[:n_occ]                # descending mass, ascending id
    if rest > 0:
        q, r = divmod(rest, n_occ)
        masses[order] += q
        masses[order[:r]] += 1
    elif rest < 0:
        spare = masses[order] - 1
        before = np.cumsum(spare) - spare
        masses[order] -= np.minimum(spare, np.maximum(-rest - before, 0))
    assert int(masses.sum()) == total and bool((masses[occurs] >= 1).all())
    return masses


def sgns_alias_table(masses):
    """(noise_keep uint32[ni], noise_alias int32[ni]) on the host: Walker / Vose alias columns of the integer `masses`
    (which sum to ``ni * 2^32``), built in integer arithmetic only, so the table represents the masses exactly:

        masses[i] = keep'[i] + sum over n != i with alias[n] == i of (2^32 - keep[n]),  keep' = 2^32 for a full column.

    Column n yields item n for a 32-bit word below ``keep[n]`` and ``alias[n]`` otherwise; a full column is stored as
    ``alias[n] == n`` (keep = 2^32 - 1).  An item of mass 0 gets keep 0 and is nobody's alias: it is never drawn.  The
    pairing is a Python loop over the ni columns -- a one-off per model: 0.11 s at ni = 200 000 with Zipf counts, measured
    on the CPU (``sgns_noise_masses`` before it: 0.27 s)."""
    rem = [int(v) for v in np.asarray(masses).reshape(-1)]
    ni = len(rem)
    if ni < 1 or min(rem) < 0 or sum(rem) != ni * NOISE_COLUMN:
        raise ValueError("masses must be non-negative and sum to ni * 2^32")
    keep, alias = [NOISE_COLUMN - 1] * ni, list(range(ni))
    small = [i for i in range(ni - 1, -1, -1) if rem[i] < NOISE_COLUMN]   # popped in ascending id
    large = [i for i in range(ni - 1, -1, -1) if rem[i] > NOISE_COLUMN]
    while small and large:
        s, l = small.pop(), large.pop()
        keep[s], alias[s] = rem[s], l
        rem[l] -= NOISE_COLUMN - rem[s]
        if rem[l] < NOISE_COLUMN:
            small.append(l)
        elif rem[l] > NOISE_COLUMN:
            large.append(l)
    assert not small and not large                                      # the masses sum to ni columns: none is left open
    return np.array(keep, np.uint32), np.array(alias, np.int32)


class SGNS(_Sequences, _SampledSGD):
    """Skip-gram with negative sampling (Mikolov, Sutskever, Chen, Corrado, Dean, NIPS 2013): word2vec for token streams,
    item2vec / prod2vec (Barkan and Koenigstein 2016; Grbovic et al. 2015) for playlists, baskets and sessions -- item
    vectors trained straight from id sequences, without users and without a co-occurrence matrix.

        model = SGNS.from_documents(indices, doc_offsets, window=5, negatives=5, rank=64)    # a document is a sequence
        losses = model.fit(steps=2000)
        ids, scores, lengths = model.similar_items(items, k=20)                     # cosine neighbours of the in rows
        rec_ids, rec_scores, rec_lengths = model.recommend_sequences(ids, offsets, k=10)     # next items of sessions

    Model.  Two tables of one rank: ``in_factors`` [ni, rank] (the centre vectors v) and ``out_factors`` [ni, rank] (the
    context vectors w).  An event is a place of a document -- the events in the order given, or by a stable sort on
    (doc, time) with `time`; repeats are kept.

    Step.  ``batch`` slots are drawn on the device (``ops.sgns_sample``: BPR's Philox counter layout): an event, its item
    the centre c; a distance d in [1, window] with weight ``window - d + 1`` (word2vec's shrunk window) on a random side,
    the item there the context o -- a slot whose context would leave the document is dropped (``valid = 0``); and
    ``negatives`` noise items from the alias table of ``counts ** power`` (``noise_keep`` / ``noise_alias``, built once
    on the host by ``sgns_alias_table``).  The objective of a step is the sum over its valid slots of
    ``softplus(-v_c . w_o) + sum_k m_k softplus(v_c . w_n_k) + (reg / 2)(|v_c|^2 + |w_o|^2 + sum_k m_k |w_n_k|^2)``,
    ``m_k = 0`` where the noise item is the context itself (word2vec skips that draw).  ``ops.sgns_fwd_bwd`` writes one
    gradient row per occurrence and the row-sparse engine updates both tables (``_SampledSGD._apply``).  The reported loss is the
    logistic part, as in the other models of this module.  The fit is a function of the inputs and the seed.
    Frequent-item subsampling (Mikolov's threshold t) is out of scope: every event is a centre with equal probability.

    ``items``: int32 ascending ids; ``counts``: int64[ni], the items' occurrence counts; the tables are ``randn *
    init_scale`` from the seeded CPU generator in the order in, out, their Adagrad accumulators ``in_accum`` /
    ``out_accum``; ``noise_keep`` holds the uint32 thresholds as int32 bits on the device; ``step``: the steps taken.
    There is no user table: ``score``, ``recommend`` and ``auc`` are refused; ``accuracy`` is the counterpart of ``auc``."""

    def __init__(self, doc, item, time=None, window=5, negatives=5, power=0.75, rank=64, reg=0.0, lr=0.05,
                 optimizer="adagrad", batch=65536, seed=0, init_scale=None, device=None):
        top_window, top_negatives, _, _ = ops.sgns_geometry()
        window, negatives, power = int(window), int(negatives), float(power)
        if not 1 <= window <= top_window:
            raise ValueError("window = %d outside [1, %d]" % (window, top_window))
        if not 1 <= negatives <= top_negatives:
            raise ValueError("negatives = %d outside [1, %d]" % (negatives, top_negatives))
        if not (math.isfinite(power) and power >= 0.0):
            raise ValueError("power = %r must be finite and not negative" % (power,))
        if time is not None:
            time = _tensor(time, "time")
            _same_length("doc, item and time", _tensor(doc, "doc"), _tensor(item, "item"), time)
        if (2 + negatives) * int(batch) > 2 ** 31 - 1:
            raise ValueError("(2 + negatives) * batch = %d gradient rows exceed 2^31 - 1" % ((2 + negatives) * int(batch)))
        doc, item = self._configure(doc, item, rank, reg, lr, optimizer, batch, seed, init_scale, device)
        self.window, self.negatives, self.power = window, negatives, power
        dev = self.device
        with torch.cuda.device(dev):
            _, upos, ipos = self._index_pairs(doc, item)
            nd, ni = int(self.users.numel()), int(self.items.numel())
            if 2 * ni > 2 ** 31 - 1:
                raise ValueError("2 ni = %d rows exceed 2^31 - 1 (the row space of the update)" % (2 * ni))
            self._set_sequences(upos, ipos, time)
            self.counts = torch.bincount(ipos, minlength=ni)
            keep, alias = sgns_alias_table(sgns_noise_masses(self.counts.cpu().numpy(), power))
            self.noise_keep = torch.from_numpy(keep.view(np.int32)).to(dev)
            self.noise_alias = torch.from_numpy(alias).to(dev)
            self.in_factors, self.out_factors, self.in_accum, self.out_accum = self._new_tables(ni, ni)

    nnz = _Sequences.n_events

    def _rows(self):
        return self.in_factors, self.out_factors

    def _no_users(self, *a, **kw):
        raise TypeError("SGNS has no user table: use similar_items, recommend_sequences and accuracy")

    score = recommend = auc = _no_users

    # ---- training -------------------------------------------------------------------------------------------------------
    def sample(self, K, step0=None, seed=None):
        """(c, e, o, valid) int32 [K, batch], neg int32 [K, batch, negatives] and dropped int32[K]: the slots of the global
        steps step0 .. step0 + K - 1 (``step0`` = the next step to take when None) -- c, o and neg positions into
        ``items``, e the centre's event number in the document CSR."""
        with torch.cuda.device(self.device):
            return ops.sgns_sample(self._seq_offsets_dev, self._seq_upos, self._seq_ipos, self.users.numel(),
                                   self.items.numel(), self.window, self.negatives, self.noise_keep, self.noise_alias,
                                   *self._stream(seed, step0), int(K), self.batch)

    def train_steps(self, K):
        """K steps: one sampler launch, then per step the forward / backward, the sort and the update over both tables.
        Returns the mean loss over the valid slots of every step (an fp64 sum of the per-slot losses divided on the host;
        NaN for a step without a valid slot).  Raises ``FactorizationError`` when a kernel met a position outside its
        table."""
        K = self._check_K(K)
        ni = int(self.items.numel())
        with torch.cuda.device(self.device):
            c, _, o, valid, neg, dropped = self.sample(K)
            # the id list of the gradient rows after the centres: [o ; neg[:, 0] ; .. ; neg[:, negatives - 1]] per step
            context = torch.cat([o[:, None, :], neg.permute(0, 2, 1)], 1).contiguous()

            def one_step(k):
                loss_t, _, grads = ops.sgns_fwd_bwd(self.in_factors, self.out_factors, c[k], o[k], neg[k], valid[k], self.reg,
                                                    failed=self._failed)
                self._apply([self.in_factors, self.out_factors], [self.in_accum, self.out_accum],
                            [c[k], context[k].reshape(-1)], [0, ni, 2 * ni], grads)
                return (loss_t.to(torch.float64).sum(),)
            sums = self._run_steps(K, "an SGNS step met a position outside its table (bit 30)", one_step)
            return _step_means(sums[0], self.batch - dropped.cpu().numpy().astype(np.int64))

    def accuracy(self, K=1, seed=None):
        """The share of (context, noise) score pairs that the model orders correctly, ``s_o > s_k``, over K * batch
        sampled slots (valid ones; a noise item that is the context itself is no pair); a tie counts half -- ``BPR.auc``'s
        convention.  The slots are steps 0 .. K - 1 of `seed` (``self.seed + 1`` when None: not a training stream, and the
        same slots before and after training).  NaN when there is no pair."""
        with torch.cuda.device(self.device):
            c, _, o, valid, neg, _ = self.sample(int(K), step0=0, seed=self.seed + 1 if seed is None else seed)
            c, o, valid, neg = c.reshape(-1), o.reshape(-1), valid.reshape(-1), neg.reshape(-1, self.negatives)
            self._failed.zero_()
            _, s, _ = ops.sgns_fwd_bwd(self.in_factors, self.out_factors, c, o, neg, valid, self.reg, want_grads=False,
                                       want_diff=True, failed=self._failed)
            self._raise_bad_position("accuracy met a position outside its table (bit 30)")
            return self._ordered_share(s[:, :1] - s[:, 1:], (valid != 0)[:, None] & (neg != o[:, None]))

    # ---- serving --------------------------------------------------------------------------------------------------------
    def item_rows(self, which="in", normalize=False):
        """float32[ni, rank]: the ``"in"`` (centre) or ``"out"`` (context) rows of every item in ``items``' order; of unit
        length (``rerank.unit_rows``) when `normalize`."""
        if which not in ("in", "out"):
            raise ValueError("which must be 'in' or 'out', got %r" % (which,))
        from . import rerank
        rows = self.in_factors if which == "in" else self.out_factors
        return rerank.unit_rows(rows) if normalize else rows.contiguous()

    def similar_items(self, items, k=20, exclude_self=True, slack=16):
        """Per query item its k nearest items by the cosine of the ``in`` rows, ordered (score descending, item id
        ascending), without the item itself when `exclude_self`: (ids int32[nq, k] padded with -1, scores float32[nq, k]
        padded with 0, lengths int32[nq]), the triple ``recommend`` returns, by its candidate scheme
        (``ops.retrieve_topk`` on the unit rows, re-scored by the predict kernel).  An unknown item gets an empty list."""
        with torch.cuda.device(self.device):
            unit = self.item_rows("in", normalize=True)
            pos = self._positions(items, self.items).to(torch.int64)
            ni = int(self.items.numel())
            own = torch.arange(ni, dtype=torch.int64, device=self.device)
            return _recommend_rows(unit, None, pos, unit, self.items, k, slack,
                                   np.arange(ni + 1, dtype=np.int64) if exclude_self else None, (own << 32) | own,
                                   lambda q: "item %d" % int(_tensor(items, "items")[q]), "is", "exclude_self")

    def _query_rows(self, ipos, offsets):
        return self._bag_rows(self.in_factors, _tail_bags(ipos, offsets, self.window, self.device), offsets.size - 1, "sequence")

    def query_rows(self, indices, doc_offsets):
        """float32[ndocs, rank]: per sequence ``indices[doc_offsets[d]:doc_offsets[d + 1]]`` the mean of the ``in`` rows of
        its last ``window`` ids that the model knows (unknown ids are skipped): ``ops.bag_sum`` with the weights
        ``float32(1 / c)``, oldest first.  A sequence without a known id gets zeros."""
        with torch.cuda.device(self.device):
            _, ipos, offsets = self._known_sequences(indices, doc_offsets)
            return self._query_rows(ipos, offsets)

    def recommend_sequences(self, indices, doc_offsets, k=500, exclude_seen=True, slack=16):
        """``recommend``'s lists for GIVEN sequences: ``query_rows`` scored against ``out_factors`` -- the items most likely
        in the context of the sequence's tail.  Sessions the model never saw are served; ids it does not know are
        skipped, as ``FPMC.recommend_sequences`` skips them.  `exclude_seen` leaves out the sequence's own items.  Returns
        (rec_ids, rec_scores, rec_lengths), what ``evaluate.ranking_metrics`` and ``diversify`` take."""
        with torch.cuda.device(self.device):
            docs, ipos, offsets = self._known_sequences(indices, doc_offsets)
            return self._recommend_sequences(self._query_rows(ipos, offsets), self.out_factors, docs, ipos, k, slack,
                                             exclude_seen)

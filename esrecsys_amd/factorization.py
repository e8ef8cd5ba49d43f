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
"""
import math

import numpy as np
import torch

from . import ops
from .ratings import _same_length, _tensor, rating_deviations
from .wikipedia.neighbours import MAX_K

CENTERS = ("user", "global", "none")
RETRIEVE_LIMIT = 1024        # the k of ops.retrieve_topk
FAIL_BAD_POSITION = 1 << 30  # esr_als.hip: a column outside the other side's table


class FactorizationError(RuntimeError):
    """A half-sweep could not solve some rows (a pivot that is not finite and positive: NaN factors handed in), or met a
    column outside the other side's table."""


def max_rank():
    """The largest rank the kernels take (esr_als_max_rank(): one wave holds a rank x rank f32 matrix in LDS)."""
    return ops.als_max_rank()


def _csr(major, minor, n_major):
    """(host row offsets int64[n_major + 1], order): the rows sorted by (major, minor) -- torch plumbing."""
    key = (major.to(torch.int64) << 32) | minor.to(torch.int64)
    key, order = torch.sort(key)
    counts = torch.bincount(major.to(torch.int64), minlength=n_major)
    offsets = np.concatenate([[0], np.cumsum(counts.cpu().numpy().astype(np.int64))]).astype(np.int64)
    return key, np.ascontiguousarray(offsets), order


class RatingsALS:
    """See the module text.  ``users`` / ``items``: int32 ascending ids; ``user_factors`` / ``item_factors``: float32
    [nu, rank] / [ni, rank]; ``user_mean``: float64[nu], the offset c."""

    def __init__(self, user, item, rating, rank=32, reg=0.1, weighted_reg=True, center="user", seed=0, init_scale=None,
                 device=None, max_rows_per_launch=None):
        rank = int(rank)
        if not 1 <= rank <= max_rank():
            raise ValueError("rank = %d outside [1, %d]" % (rank, max_rank()))
        reg = float(reg)
        if not (math.isfinite(reg) and reg > 0.0 and float(np.float32(reg)) > 0.0 and math.isfinite(float(np.float32(reg)))):
            raise ValueError("reg = %r must be finite and positive (a row with fewer ratings than rank is singular "
                             "without it)" % (reg,))
        if center not in CENTERS:
            raise ValueError("center must be 'user', 'global' or 'none', got %r" % (center,))
        if max_rows_per_launch is not None and int(max_rows_per_launch) < 1:
            raise ValueError("max_rows_per_launch = %r below 1" % (max_rows_per_launch,))
        user, item, rating = _tensor(user, "user"), _tensor(item, "item"), _tensor(rating, "rating")
        _same_length("user, item and rating", user, item, rating)
        if user.dtype.is_floating_point or item.dtype.is_floating_point:
            raise TypeError("user and item must be integer arrays")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("device must be a CUDA/ROCm device (no CPU fallback exists)")
        self.rank, self.reg, self.weighted_reg, self.center, self.seed = rank, reg, bool(weighted_reg), center, int(seed)
        self.max_rows_per_launch = None if max_rows_per_launch is None else int(max_rows_per_launch)
        self.init_scale = float(rank) ** -0.5 if init_scale is None else float(init_scale)
        dev = self.device
        with torch.cuda.device(dev):
            user, item = user.to(dev).to(torch.int64), item.to(dev).to(torch.int64)
            rating64 = rating.to(device=dev, dtype=torch.float64)
            if user.numel() and (int(user.min()) < 0 or int(item.min()) < 0 or int(user.max()) >= 2 ** 31 - 1
                                 or int(item.max()) >= 2 ** 31 - 1):
                raise ValueError("user and item ids must lie in [0, 2^31 - 1)")
            users, upos = torch.unique(user, return_inverse=True)
            items, ipos = torch.unique(item, return_inverse=True)
            nu, ni = int(users.numel()), int(items.numel())
            self.users, self.items = users.to(torch.int32).contiguous(), items.to(torch.int32).contiguous()
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
            key, self._user_offsets, order = _csr(upos, ipos, nu)
            if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
                raise ValueError("a (user, item) is rated twice: keep one rating per pair (latest_ratings)")
            self._key = key                                             # upos << 32 | ipos, ascending: the training pairs
            self._row_upos = (key >> 32).to(torch.int32).contiguous()
            self._row_ipos = (key & 0xFFFFFFFF).to(torch.int32).contiguous()
            self._targets = d[order].contiguous()
            _, self._item_offsets, order_i = _csr(ipos, upos, ni)
            self._col_upos = upos[order_i].to(torch.int32).contiguous()
            self._targets_by_item = d[order_i].contiguous()
            gen = torch.Generator(device="cpu").manual_seed(self.seed)
            self.item_factors = (torch.randn(ni, rank, generator=gen) * self.init_scale).to(dev).contiguous()
            self.user_factors = torch.zeros(nu, rank, dtype=torch.float32, device=dev)
            self._failed = torch.zeros(1, dtype=torch.int32, device=dev)

    nnz = property(lambda self: int(self._targets.numel()))

    # ---- the fit --------------------------------------------------------------------------------------------------------
    def _half_sweep(self, other, offsets, cols, targets, out, side):
        n_rows = offsets.size - 1
        step = n_rows if self.max_rows_per_launch is None else self.max_rows_per_launch
        with torch.cuda.device(self.device):
            self._failed.zero_()
            for a in range(0, n_rows, max(step, 1)):
                ops.als_solve_rows(other, offsets, cols, targets, a, min(a + step, n_rows), self.reg, self.weighted_reg, out,
                                   self._failed)
            word = int(self._failed.item())
        if word & FAIL_BAD_POSITION:
            raise FactorizationError("the %s half-sweep met a position outside the other side's table" % side)
        if word:
            raise FactorizationError("the %s half-sweep could not solve %d row(s): a pivot that is not finite and positive "
                                     "(are the other side's factors finite?); those rows were left unchanged" % (side, word))

    def solve_users(self):
        self._half_sweep(self.item_factors, self._user_offsets, self._row_ipos, self._targets, self.user_factors, "user")

    def solve_items(self):
        self._half_sweep(self.user_factors, self._item_offsets, self._col_upos, self._targets_by_item, self.item_factors,
                         "item")

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

    # ---- prediction -----------------------------------------------------------------------------------------------------
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

    def predict(self, users, items):
        """float32[nq]: ``float32(c[u] + x_u . y_i)``; NaN where the user or the item is unknown."""
        users, items = _tensor(users, "users"), _tensor(items, "items")
        _same_length("users and items", users, items)
        with torch.cuda.device(self.device):
            return ops.als_predict(self.user_factors, self.item_factors, self._positions(users, self.users),
                                   self._positions(items, self.items), offset=self.user_mean)

    def residuals(self):
        """float32[nnz]: ``float32(float64(d) - x_u . y_i)`` of the training pairs in CSR-by-user order."""
        with torch.cuda.device(self.device):
            return ops.als_predict(self.user_factors, self.item_factors, self._row_upos, self._row_ipos, targets=self._targets)

    def objective(self):
        """J of the module text, an fp64 reduction (python float)."""
        with torch.cuda.device(self.device):
            res = self.residuals().to(torch.float64)
            wu = torch.from_numpy(np.diff(self._user_offsets)).to(self.device).to(torch.float64)
            wi = torch.from_numpy(np.diff(self._item_offsets)).to(self.device).to(torch.float64)
            if not self.weighted_reg:
                wu, wi = torch.ones_like(wu), torch.ones_like(wi)
            xu = (self.user_factors.to(torch.float64) ** 2).sum(1)
            yi = (self.item_factors.to(torch.float64) ** 2).sum(1)
            return float((res * res).sum() + self.reg * (wu * xu).sum() + self.reg * (wi * yi).sum())

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
        k, slack = int(k), int(slack)
        if not 1 <= k <= MAX_K:
            raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
        if slack < 0:
            raise ValueError("slack = %d is negative" % slack)
        dev = self.device
        with torch.cuda.device(dev):
            upos = self._positions(users, self.users).to(torch.int64)
            nq, ni = int(upos.numel()), int(self.items.numel())
            ids = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
            scores = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            lengths = torch.zeros(nq, dtype=torch.int32, device=dev)
            if nq == 0 or ni == 0:
                return ids, scores, lengths
            known = upos >= 0
            safe = upos.clamp(min=0)
            r_max = 0
            if exclude_rated and bool(known.any()):
                lens = torch.from_numpy(np.diff(self._user_offsets)).to(dev)
                rated = torch.where(known, lens[safe], torch.zeros_like(safe))
                r_max = int(rated.max())
                if k + r_max + slack > RETRIEVE_LIMIT and ni > RETRIEVE_LIMIT:
                    q = int(torch.argmax(rated))
                    raise ValueError("query %d (user %d) rated %d items: k + rated + slack = %d candidates exceed the %d "
                                     "that retrieve_topk selects; lower k or query that user without exclude_rated"
                                     % (q, int(_tensor(users, "users")[q]), r_max, k + r_max + slack, RETRIEVE_LIMIT))
            kc = min(ni, k + r_max + slack)
            if kc > RETRIEVE_LIMIT:
                raise ValueError("query 0: k + slack = %d candidates exceed the %d that retrieve_topk selects"
                                 % (k + slack, RETRIEVE_LIMIT))
            queries = torch.where(known[:, None], self.user_factors[safe], torch.zeros((), device=dev)).contiguous()
            _, cand = ops.retrieve_topk(queries, self.item_factors, kc, mode="exact")          # [nq, kc] item positions
            cand = cand.to(torch.int64)
            sc = ops.als_predict(self.user_factors, self.item_factors,
                                 upos[:, None].expand(nq, kc).to(torch.int32).contiguous().reshape(-1),
                                 cand.to(torch.int32).contiguous().reshape(-1), offset=self.user_mean).reshape(nq, kc)
            drop = ~known[:, None].expand(nq, kc)
            if exclude_rated and self._key.numel():
                pair = (safe[:, None] << 32) | cand
                at = torch.searchsorted(self._key, pair.reshape(-1)).clamp(max=self._key.numel() - 1).reshape(nq, kc)
                drop = drop | (self._key[at] == pair)
            # (score descending, item ascending): positions ascend with ids; dropped candidates go last
            by_item = torch.sort(cand, dim=1, stable=True)
            sc_i, drop_i = torch.gather(sc, 1, by_item.indices), torch.gather(drop, 1, by_item.indices)
            rank_key = torch.where(drop_i, torch.full_like(sc_i, -float("inf")), sc_i)
            by_score = torch.sort(rank_key, dim=1, descending=True, stable=True)
            live = (~torch.gather(drop_i, 1, by_score.indices))[:, :k]
            kk = min(k, kc)
            top_items = torch.gather(by_item.values, 1, by_score.indices)[:, :kk]
            top_scores = torch.gather(sc_i, 1, by_score.indices)[:, :kk]
            ids[:, :kk] = torch.where(live, self.items[top_items], torch.full_like(ids[:, :kk], -1))
            scores[:, :kk] = torch.where(live, top_scores, torch.zeros_like(top_scores))
            lengths = live.sum(1).to(torch.int32)
            return ids, scores, lengths

"""Offline evaluation: a hold-out split of id documents and the ranking metrics of recommended lists against the held-out
ids, on the GPU (esr_eval.hip).

    context, c_off, truth, t_off, kept = split_holdout(indices, doc_offsets)       # first 5 ids in, the rest held out
    table = neighbours(*DiceBuilder().add(context, c_off).finalize(), ...)          # any recommender built on the contexts
    rec_ids, _, rec_lengths = recommend(table, context, c_off, k=500)
    m = ranking_metrics(rec_ids, rec_lengths, truth, t_off, ks=(10, 100, 500))
    m.mean()["recall"]                                                              # float64 [3], over the valid queries

The protocol is the reference's (``spotify/make_training.py:74-98``): the first ``context`` ids of a document are what the
recommender sees, the rest are to be predicted, and documents below ``min_length`` ids are dropped; its trainer reports the
recall of the next tracks among the 500 best (``train_spotify.py:113-131``), which is ``ranking_metrics(..., ks=(500,),
count_repeats=True, truth_size="listed").hits / listed length``.

Definitions, per query and cutoff k, with kmax = min(ks[-1], width).  Position r (1-based) <= min(length, kmax) is a hit if
its id is a truth id and -- unless ``count_repeats`` -- no earlier position holds the same id: a repeated recommendation
counts once, at its first rank.  c = the hits at ranks <= k; n_rel = the number of DISTINCT truth ids
(``truth_size="distinct"``) or the listed length (``"listed"``, the reference's ``numel``).

    precision = c / k        recall = c / n_rel        rr = 1 / first_hit if first_hit <= k else 0
    ap   = (sum over the hits at ranks r <= k of (hits up to r) / r) / min(k, n_rel)
    ndcg = (sum over the hits at ranks r <= k of 1 / log2(r + 1)) / (sum over r <= min(k, n_rel) of 1 / log2(r + 1))

Each is computed in float64 in ascending rank order and rounded once to float32; the discount table and its running sum are
made here with NumPy in float64 and uploaded, so the device's bits are those of a NumPy restatement.  A query without truth
ids gets zeros and ``valid == 0``; ``mean()`` leaves it out.  With ``count_repeats`` the hits may exceed n_rel, so ``ap``
and ``ndcg`` are None.
"""
import numpy as np
import torch

from . import ops
from .wikipedia.pair_table import csr_inputs, failure_text

MAX_CUTOFFS = 8
FAILURES = {2: "a negative truth id", 4: "truth_offsets changed between the host's check and the launch",
            8: "a query with more distinct truth ids than the table in LDS takes"}
_FLOATS = ("precision", "recall", "rr", "ap", "ndcg")


class EvaluationError(ValueError):
    """The device raised the failure word of esr_eval_ranking: the truth ids are not what the call was told."""


def max_truth():
    """Distinct truth ids one query may hold (esr_eval_max_truth(): a workgroup keeps them in a table in LDS)."""
    return ops.eval_max_truth()


def max_width():
    """The widest recommended list that is scored (esr_eval_max_width())."""
    return ops.eval_max_width()


def discount_tables(kmax, kideal):
    """(disc float64[kmax], cum_disc float64[kideal + 1]): disc[r - 1] = 1 / log2(r + 1) and cum_disc = [0, cumsum] of the
    same discounts continued to kideal -- the two tables the kernel reads and a restatement must use."""
    n = max(int(kmax), int(kideal))
    disc = 1.0 / np.log2(np.arange(2, n + 2, dtype=np.float64))
    cum = np.concatenate([np.zeros(1), np.cumsum(disc)])
    return disc[:kmax].copy(), cum[:kideal + 1].copy()


class RankingMetrics:
    """Per-query device tensors: ``hits int32[nq, nk]``, ``first_hit int32[nq]`` (1-based, 0 = none within kmax),
    ``valid int32[nq]``, ``precision`` / ``recall`` / ``rr`` / ``ap`` / ``ndcg float32[nq, nk]`` (``ap`` and ``ndcg`` None
    with count_repeats), and ``ks`` as given."""

    def __init__(self, ks, tensors):
        self.ks = tuple(ks)
        for name, t in tensors.items():
            setattr(self, name, t)

    def mean(self):
        """{"precision": float64[nk], ..., "n_valid": int}: every float metric averaged over the valid queries, summed
        in query order in float64 on a host copy (nq numbers per column: plumbing, not the hot path).  Zeros when no
        query is valid."""
        valid = self.valid.cpu().numpy() != 0
        n_valid = int(valid.sum())
        out = {"n_valid": n_valid}
        for name in _FLOATS:
            t = getattr(self, name)
            if t is None:
                out[name] = None
                continue
            x = np.ascontiguousarray(t.cpu().numpy().astype(np.float64)[valid])
            out[name] = np.add.reduce(x, axis=0) / n_valid if n_valid else np.zeros(len(self.ks))
        return out


def _check_ks(ks):
    try:
        ks = tuple(int(k) for k in ks)
    except TypeError:
        raise TypeError("ks must be a sequence of ints, got %r" % (ks,))
    if not 1 <= len(ks) <= MAX_CUTOFFS:
        raise ValueError("ks holds %d cutoffs, outside [1, %d]" % (len(ks), MAX_CUTOFFS))
    for j, k in enumerate(ks):
        if k < 1 or k > 2 ** 31 - 1 or (j and k <= ks[j - 1]):
            raise ValueError("ks must be strictly ascending cutoffs >= 1, got %r" % (ks,))
    return ks


_tables = {}


def ranking_metrics(rec_ids, rec_lengths, truth, truth_offsets, ks=(10, 100, 500), count_repeats=False,
                    truth_size="distinct"):
    """The ``RankingMetrics`` of the lists ``rec_ids int32[nq, width]`` (device; ``-1`` behind a row's end and
    ``rec_lengths int32[nq]`` or None for full rows -- what ``recommend`` returns) against the truth sets
    ``truth[truth_offsets[q]:truth_offsets[q + 1]]`` (int32 ids with int64 CSR offsets, host or device).  See the module
    text for the definitions.  One launch (esr_eval_ranking) and one read of its failure word.

    Refused before any launch, with the query named: a list wider than ``max_width()``, a query with more than
    ``max_truth()`` distinct truth ids (never truncated), ``ks`` that is not 1 to 8 strictly ascending cutoffs, shapes that
    disagree, CPU lists.  A negative truth id raises ``EvaluationError`` after the launch, as the pair-table builders do."""
    ks = _check_ks(ks)
    if truth_size not in ("distinct", "listed"):
        raise ValueError("truth_size must be 'distinct' or 'listed', got %r" % (truth_size,))
    if not isinstance(rec_ids, torch.Tensor) or not rec_ids.is_cuda:
        raise TypeError("rec_ids must be a CUDA/ROCm tensor (no CPU fallback exists)")
    if rec_ids.dim() != 2:
        raise ValueError("rec_ids must be [nq, width], got shape %s" % (tuple(rec_ids.shape),))
    dev, (nq, width) = rec_ids.device, rec_ids.shape
    if not 1 <= width <= max_width():
        raise ValueError("list width %d outside [1, %d]" % (width, max_width()))
    if rec_lengths is not None:
        if not isinstance(rec_lengths, torch.Tensor) or not rec_lengths.is_cuda:
            raise TypeError("rec_lengths must be a CUDA/ROCm tensor or None (no CPU fallback exists)")
        if rec_lengths.numel() != nq:
            raise ValueError("rec_lengths holds %d lengths for %d lists" % (rec_lengths.numel(), nq))
    with torch.cuda.device(dev):
        truth, off_host, off_dev = csr_inputs(truth, truth_offsets, dev, "truth")
        if off_host.size - 1 != nq:
            raise ValueError("truth_offsets describes %d truth sets for %d lists" % (off_host.size - 1, nq))
        lens = np.diff(off_host)
        cap = max_truth()
        for q in np.flatnonzero(lens > cap):      # rare: only a set listed above the cap can hold too many distinct ids
            distinct = int(torch.unique(truth[off_host[q]:off_host[q + 1]]).numel())
            if distinct > cap:
                raise ValueError("query %d has %d distinct truth ids, above the cap of %d per query (esr_eval.hip keeps "
                                 "a query's truth in LDS); nothing is truncated" % (int(q), distinct, cap))
        longest = int(lens.max()) if nq else 0
        if longest > 2 ** 31 - 1:
            raise ValueError("a truth set of %d ids" % longest)
        if rec_ids.dtype != torch.int32 or (width > 1 and rec_ids.stride(1) != 1):
            rec_ids = rec_ids.to(torch.int32).contiguous()
        if rec_lengths is not None:
            rec_lengths = ops.as_ids(rec_lengths, dev).reshape(-1)
        kmax, kideal = min(ks[-1], width), min(ks[-1], longest)
        key = (kmax, kideal, dev)
        if key not in _tables:
            if len(_tables) > 64:
                _tables.clear()
            _tables[key] = tuple(torch.from_numpy(t).to(dev) for t in discount_tables(kmax, kideal))
        disc, cum = _tables[key]
        out, fail = ops.eval_ranking(rec_ids, rec_lengths, truth, off_dev, longest, ks, disc, cum, count_repeats,
                                     truth_size == "listed")
    if fail:
        raise EvaluationError("ranking metrics failure (bits %d): %s" % (fail, failure_text(fail, FAILURES)))
    return RankingMetrics(ks, out)


def split_holdout(indices, doc_offsets, context=5, min_length=10, mode="first"):
    """The reference's hold-out protocol at id level (``spotify/make_training.py:74-98``): documents
    ``indices[doc_offsets[d]:doc_offsets[d + 1]]`` shorter than `min_length` are dropped; of each kept one the first
    `context` ids are the context and the rest the truth (``mode="first"``), or the last `context` ids are held out as
    the truth and the ids before them are the context (``mode="last"``, leave-last-n-out).

    Returns ``(context, context_offsets, truth, truth_offsets, kept)``: ids int32 and CSR offsets int64 on the input's
    device (host arrays become CPU tensors), ``kept int64`` the surviving document numbers in order.  `min_length` must
    exceed `context` (the reference's ``assert len(next_track) > 0``).  Index arithmetic in torch: not a hot path."""
    context, min_length = int(context), int(min_length)
    if mode not in ("first", "last"):
        raise ValueError("mode must be 'first' or 'last', got %r" % (mode,))
    if context < 1 or min_length <= context:
        raise ValueError("need 1 <= context < min_length, got context=%d min_length=%d" % (context, min_length))
    ids = indices if isinstance(indices, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(indices)))
    dev = ids.device
    ids = ids.reshape(-1).to(torch.int32)
    off = doc_offsets if isinstance(doc_offsets, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(np.asarray(doc_offsets), dtype=np.int64))
    off = off.reshape(-1).to(device=dev, dtype=torch.int64)
    if off.numel() < 1:
        raise ValueError("doc_offsets must be int64 [ndocs + 1]")
    lens = off[1:] - off[:-1]
    if off.numel() > 1 and (int(off[0]) != 0 or int(off[-1]) != ids.numel() or bool((lens < 0).any())):
        raise ValueError("doc_offsets must rise from 0 to len(indices) = %d" % ids.numel())
    kept = torch.nonzero(lens >= min_length).reshape(-1)
    start, length = off[kept], lens[kept]
    fixed = torch.full_like(length, context)
    if mode == "first":
        parts = ((start, fixed), (start + context, length - context))
    else:
        parts = ((start, length - context), (start + length - context, fixed))
    out = []
    for begin, n in parts:
        o = torch.zeros(n.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n, 0, out=o[1:])
        total = int(o[-1]) if n.numel() else 0
        at = torch.repeat_interleave(begin - o[:-1], n) + torch.arange(total, dtype=torch.int64, device=dev)
        out += [ids[at], o]
    return out[0], out[1], out[2], out[3], kept


def split_last(indices, doc_offsets, n_last=1, min_length=3):
    """The leave-last-out protocol of next-item evaluation: of every document of at least `min_length` ids the last `n_last`
    are the truth and everything before them, in order, the training sequence (``factorization.FPMC.from_documents`` takes
    it as it is).  Returns what ``split_holdout`` returns -- ``(context, context_offsets, truth, truth_offsets, kept)`` --
    so the truth goes straight into ``ranking_metrics``; `min_length` must exceed `n_last`."""
    n_last, min_length = int(n_last), int(min_length)
    if n_last < 1 or min_length <= n_last:
        raise ValueError("need 1 <= n_last < min_length, got n_last=%d min_length=%d" % (n_last, min_length))
    return split_holdout(indices, doc_offsets, context=n_last, min_length=min_length, mode="last")

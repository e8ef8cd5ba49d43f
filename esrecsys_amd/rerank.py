"""Diversity re-ranking between ``recommend`` and the metrics (esr_rerank.hip): Maximal Marginal Relevance (Carbonell and
Goldstein, SIGIR 1998) cuts the final list from a longer candidate list by trading relevance against redundancy, and
intra-list similarity (Ziegler et al., WWW 2005) measures how alike the items of a list are.

    rec_ids, rec_scores, rec_lengths = model.recommend(users, k=500)
    div_ids, div_scores, div_lengths = model.diversify(rec_ids, rec_scores, rec_lengths, lam=0.7, n=100)
    m = ranking_metrics(div_ids, div_lengths, truth, truth_offsets, ks=(10, 100))
    pos = model._positions(div_ids.reshape(-1), model.items).reshape(div_ids.shape)          # ids -> row positions
    ils = intra_list_similarity(pos, div_lengths, unit_rows(model.item_factors), ks=(10, 100)).mean()

The rule is stated in ``csrc/esr_rerank_rule.h``.  A list is ``cand int32[nq, width]`` of item POSITIONS into ``rows
float32[ni, D]`` with ``rel float32[nq, width]`` and ``lengths int32[nq]`` (or None: full rows).  Round t of ``mmr`` picks
the candidate with the greatest ``lam * rel - (1 - lam) * max sim to the rows picked before`` (the similarity is the dot
product of the rows: cosine on ``unit_rows``), ties to the earlier list position; ``lam = 1`` is the stable sort by rel.
One kernel call per function and one read of its failure word; ``unit_rows`` and ``coverage`` are torch plumbing.
"""
import numpy as np
import torch

from . import ops
from .evaluate import _check_ks

FAIL_BAD_POSITION = 1 << 30   # esr_rerank_rule.h kRerankFailPos: a candidate position outside the rows
FAIL_BAD_REL = 1 << 29        # kRerankFailRel: a relevance that is not finite


class RerankError(RuntimeError):
    """A list held a candidate position outside the row table (bit 30) or a relevance that is not finite (bit 29)."""


def _raise_failed(word, who):
    if word & FAIL_BAD_POSITION:
        raise RerankError("%s: a candidate position inside a list's length lies outside the rows (bit 30)" % who)
    if word & FAIL_BAD_REL:
        raise RerankError("%s: a relevance inside a list's length is not finite (bit 29)" % who)


def _failure_word(rows, cand):
    """A zeroed failure word beside `rows`; host tensors are refused here, before a device is asked for anything."""
    ops._req(rows, torch.float32, "rows"), ops._req(cand, torch.int32, "cand")
    return torch.zeros(1, dtype=torch.int32, device=rows.device)


def mmr(cand, rel, lengths, rows, lam=0.7, n=None):
    """(items int32[nq, n], rel float32[nq, n], lengths int32[nq], pos int32[nq, n], value float32[nq, n]): per query the n
    (default: the width) picks of MMR in pick order -- the item position, its rel, the picks made, the position within the
    candidate list and the MMR value it was picked at; -1 / 0 / . / -1 / 0 behind a list's end."""
    failed = _failure_word(rows, cand)
    n = int(cand.shape[-1]) if n is None else n
    with torch.cuda.device(rows.device):
        pos, items, out_rel, value, out_len = ops.rerank_mmr(rows, cand, rel, lengths, lam, n, failed=failed)
    _raise_failed(int(failed.item()), "mmr")
    return items, out_rel, out_len, pos, value


class IntraListSimilarity:
    """``ils float32[nq, nk]`` and ``valid int32[nq, nk]`` (device) at the cutoffs ``ks``."""

    def __init__(self, ks, ils, valid):
        self.ks, self.ils, self.valid = tuple(ks), ils, valid

    def mean(self):
        """{"ils": float64[nk], "n_valid": int64[nk]}: per cutoff the mean over the queries valid there, summed in query
        order in float64 on a host copy (as ``RankingMetrics.mean``); 0 where no query is valid."""
        ils, valid = self.ils.cpu().numpy().astype(np.float64), self.valid.cpu().numpy() != 0
        n = valid.sum(0).astype(np.int64)
        total = np.array([np.sum(ils[valid[:, j], j], dtype=np.float64) for j in range(len(self.ks))], np.float64)
        return {"ils": np.where(n > 0, total / np.maximum(n, 1), 0.0), "n_valid": n}


def intra_list_similarity(cand, lengths, rows, ks=(10, 100)):
    """The ``IntraListSimilarity`` of the lists ``cand`` (item positions into ``rows``; ``lengths`` or None) at the cutoffs
    ``ks``: the mean similarity over the pairs among a list's first min(k, length) candidates; a list with fewer than two is
    not valid at that cutoff."""
    ks = _check_ks(ks)
    failed = _failure_word(rows, cand)
    with torch.cuda.device(rows.device):
        ils, valid = ops.rerank_ils(rows, cand, lengths, ks, failed=failed)
    _raise_failed(int(failed.item()), "intra_list_similarity")
    return IntraListSimilarity(ks, ils, valid)


def unit_rows(table):
    """float32 rows of `table` divided by their Euclidean norm: the norm in fp64, one rounding; a zero row stays zero."""
    t = table.to(torch.float64)
    norm = torch.sqrt((t * t).sum(1, keepdim=True))
    return torch.where(norm > 0, t / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(t)) \
        .to(torch.float32).contiguous()


def coverage(rec_ids, rec_lengths, ks):
    """int64[nk] (host): the distinct ids among the first min(k, length) entries of all lists ``rec_ids [nq, width]``
    (``rec_lengths`` or None: full rows), per cutoff of ``ks``."""
    ks = _check_ks(ks)
    nq, width = rec_ids.shape
    col = torch.arange(width, device=rec_ids.device)[None, :]
    live = col < (rec_lengths.to(torch.int64)[:, None] if rec_lengths is not None else width)
    return np.array([int(torch.unique(rec_ids[(live & (col < k)).expand(nq, width)]).numel()) for k in ks], np.int64)

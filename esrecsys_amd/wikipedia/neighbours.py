"""Item-to-item neighbours from a co-occurrence matrix, and the item-kNN recommender over them -- the consumer of the
pair tables that the reference has in ``wikipedia/dump_dice.py`` (the best partners of an item by Dice score; the same
arithmetic as ``train_txt2url.py``'s ``url_triplet_generator``), on the GPU (esr_neighbours.hip).

    builder = DiceBuilder().add(indices, doc_offsets)           # playlists as documents of track ids, baskets, page links
    index, other, count = builder.finalize()
    ids, df = builder.doc_frequency()
    table = neighbours(index, other, count, ids, df, k=20)      # per item its 20 best partners
    rec_ids, rec_scores, rec_lengths = recommend(table, history, offsets, k=500)   # per query (a set of items)

Row of item x: ``orientation="stored"`` takes the entries with ``index == x`` -- the row the reference dumps;
``orientation="both"`` those with ``index == x`` or ``other == x`` and the partner at the other end -- the symmetric
matrix that the half table stands for.  ``score="dice"`` is ``count / (df[other] + df[index])`` in f32, without the
textbook factor 2 (dump_dice.py:45), the bits of ``make_dice.dice_scores``; ``score="count"`` is the joint count.

Order inside a row: score descending, then partner id ascending -- the project's rule that ties go to the lower index.
DEVIATION from the reference: dump_dice.py:46-48 sorts ``(dice, joint_count, title)`` tuples in reverse, so it breaks
score ties by the larger joint count and then by the later title string.  Titles do not exist at id level; here the id
decides.  The order is total, so a table is a pure function of its input: atomic order, grid size and how the work is
cut into launches cannot show.
"""
import numpy as np
import torch

from .. import ops
from .pair_table import FAILURES as TABLE_FAILURES, CooccurrenceError, failure_text, host_offsets

MAX_K = 1024      # the cap of the project's select kernels
FAILURES = dict(TABLE_FAILURES)
FAILURES[64] = "an entry with an id that `ids` does not hold"


class NeighbourTable:
    """The k best partners of every id, device tensors: ``ids int32[u]`` (ascending; row r belongs to ids[r]),
    ``neighbours int32[u, k]`` (-1 behind a row's end), ``scores`` / ``counts float32[u, k]`` (0 there; counts = the joint
    count of each kept partner), ``lengths int32[u]`` = min(k, row length).  ``orientation`` and ``score`` as given."""

    def __init__(self, ids, neighbours, scores, counts, lengths, orientation, score):
        self.ids, self.neighbours, self.scores, self.counts, self.lengths = ids, neighbours, scores, counts, lengths
        self.orientation, self.score = orientation, score

    k = property(lambda self: int(self.neighbours.shape[1]))

    def row(self, x):
        """(partners, scores, counts) of item x as host arrays; empty for an id without entries.  KeyError when the
        table has no such id."""
        ids = self.ids.cpu().numpy()
        r = int(np.searchsorted(ids, x))
        if r >= ids.size or ids[r] != x:
            raise KeyError(x)
        n = int(self.lengths[r])
        return (self.neighbours[r, :n].cpu().numpy(), self.scores[r, :n].cpu().numpy(), self.counts[r, :n].cpu().numpy())


def plan_bounds():
    """The row lengths at which the select kernel changes class (esr_neighbours_plan_bounds), ascending."""
    return ops.neighbours_plan_bounds()


def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k = %d outside [1, %d]" % (k, MAX_K))
    return k


def neighbours(index, other, count, ids, df, k, orientation="both", score="dice"):
    """The per-row top-k neighbour table of the matrix (index, other, count) -- what ``DiceBuilder.finalize()`` or
    ``CooccurrenceBuilder.finalize()`` return: device tensors holding ONE orientation of every pair, either one.

    (ids, df) as ``DiceBuilder.doc_frequency()`` returns them: ids ascending (they may be sparse, up to 2^31 - 2), df
    their document frequencies -- required for ``score="dice"``.  For ``score="count"`` ids alone is needed, and when it
    is None the sorted distinct ids that occur are used.  An entry whose end is not in ids raises ``CooccurrenceError``.
    See the module text for rows, scores and the order (and its deviation from the reference's tie-break)."""
    k = _check_k(k)
    if orientation not in ("stored", "both"):
        raise ValueError("orientation must be 'stored' or 'both', got %r" % (orientation,))
    if score not in ("dice", "count"):
        raise ValueError("score must be 'dice' or 'count', got %r" % (score,))
    if score == "dice" and (ids is None or df is None):
        raise ValueError("score='dice' needs ids and df (DiceBuilder.doc_frequency())")
    if not isinstance(index, torch.Tensor) or not index.is_cuda:
        raise TypeError("index must be a CUDA/ROCm tensor (no CPU fallback exists)")
    dev = index.device
    with torch.cuda.device(dev):
        index, other = ops.as_ids(index, dev).reshape(-1), ops.as_ids(other, dev).reshape(-1)
        count = ops.as_f32(count, dev).reshape(-1)
        if not index.numel() == other.numel() == count.numel():
            raise ValueError("index, other and count must have one length")
        if ids is None:
            ids = torch.unique(torch.cat([index, other]))   # sorted; plumbing, not the hot path
        ids = ops.as_ids(ids, dev).reshape(-1)
        if score == "dice":
            df = ops.as_f32(df, dev).reshape(-1)
            if df.numel() != ids.numel():
                raise ValueError("ids and df must have one length")
        else:
            df = None
        nb, scores, counts, lengths, fail = ops.neighbours_topk(index, other, count, ids, df, k, orientation == "both",
                                                                score == "dice")
    if fail:
        raise CooccurrenceError("neighbour table failure (bits %d): %s" % (fail, failure_text(fail, FAILURES)))
    return NeighbourTable(ids, nb, scores, counts, lengths, orientation, score)


def dump_dice(table, title_of, max_rows=20):
    """The lines dump_dice.py:33-51 prints, from a ``"stored"`` / ``"dice"`` table: for each of the first `max_rows`
    rows that have entries (the rows of the matrix file, ascending by id) ``"Nearest to %s"`` and then its partners as
    ``"\\tScore %f joint count %d url %s"``.  The reference's quirk is kept: a row prints ``min(max_rows, len)``
    partners, not ``max_terms`` (and here never more than the table's k).  `title_of`: id -> title, a mapping or a
    callable.  Host formatting only; the order of tied scores is the table's (see the module text)."""
    if table.orientation != "stored" or table.score != "dice":
        raise ValueError("dump_dice prints a table made with orientation='stored', score='dice'")
    title = title_of if callable(title_of) else title_of.__getitem__
    lengths = table.lengths.cpu().numpy()
    rows = np.flatnonzero(lengths > 0)[:max_rows]
    ids = table.ids.cpu().numpy()
    lines = []
    if rows.size == 0:
        return lines
    sel = torch.from_numpy(rows).to(table.ids.device)
    nb, sc, ct = (t[sel].cpu().numpy() for t in (table.neighbours, table.scores, table.counts))
    for i, r in enumerate(rows):
        lines.append("Nearest to %s" % title(int(ids[r])))
        for j in range(min(max_rows, int(lengths[r]))):
            lines.append("\tScore %f joint count %d url %s" % (float(sc[i, j]), int(ct[i, j]), title(int(nb[i, j]))))
    return lines


def max_entries():
    """History length x table width one query may gather (esr_itemknn_max_entries(): a workgroup sorts them in LDS)."""
    return ops.itemknn_max_entries()


def recommend(table, history, offsets, k, exclude_history=True):
    """Item-kNN: for query q = ``history[offsets[q]:offsets[q + 1]]`` (int32 ids with int64 CSR offsets, the layout the
    builders' ``add`` takes) the k best candidates as (rec_ids int32[nq, k] padded with -1, rec_scores float32[nq, k]
    padded with 0, rec_lengths int32[nq]).

    The score of candidate c is the f32 sum of ``table.scores[row(h_p), j]`` over the history positions p and columns j
    with ``table.neighbours[row(h_p), j] == c``, accumulated left to right in ascending position order -- the kernel sorts
    a query's gathered entries by (candidate, position) and sums each run in that order, so the result is
    bit-reproducible.  A repeated history id counts once per occurrence, an id the table lacks adds nothing, and with
    `exclude_history` candidates that occur in the query's history are dropped.  Order: score descending, id ascending.

    A query gathers history length x table.k entries, at most ``max_entries()``; a longer one raises ``ValueError`` before
    any launch and is never truncated (the ``MAX_DOC`` policy of ``make_dice``)."""
    k = _check_k(k)
    dev = table.ids.device
    n = history.numel() if isinstance(history, torch.Tensor) else np.asarray(history).size
    off_host = host_offsets(offsets, n, "history")
    cap, width = max_entries(), table.k
    lens = np.diff(off_host)
    over = np.flatnonzero(lens * width > cap)
    if over.size:
        q = int(over[0])
        raise ValueError("query %d has %d history ids x table width %d = %d entries, above the cap of %d entries per query "
                         "(esr_neighbours.hip sorts a query in LDS); shorten the history or build a narrower table"
                         % (q, int(lens[q]), width, int(lens[q]) * width, cap))
    with torch.cuda.device(dev):
        history = ops.as_ids(history.to(dev) if isinstance(history, torch.Tensor) else history, dev).reshape(-1)
        if isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.dtype == torch.int64 and \
                offsets.is_contiguous() and offsets.device == dev:
            off_dev = offsets
        else:
            off_dev = torch.from_numpy(off_host).to(dev)
        return ops.itemknn_recommend(table.ids, table.neighbours, table.scores, table.lengths, history, off_dev, k,
                                     exclude_history)

"""Makes the set co-occurrence (Dice) matrix -- the reference's ``wikipedia/make_dice.py`` (a PySpark job there, scored by
``dump_dice.py``) on the GPU, from id sets: baskets, sessions, playlists, page-link sets.

The input is ``indices int32[N]`` with ``doc_offsets int64[ndocs + 1]`` (CSR, as ``CooccurrenceBuilder.add`` takes it):
document d is ``indices[doc_offsets[d]:doc_offsets[d + 1]]`` -- its primary index followed by its secondary indices.  Only
the set matters.

    builder = DiceBuilder()
    builder.add(indices, doc_offsets)           # any number of times: the reduce-by-key over the corpus
    index, other, count = builder.finalize()    # device tensors, ascending by (index, other), index < other
    ids, df = builder.doc_frequency()           # documents per id
    write_cooccurrence(path, index, other, count)               # the reference's *.cooccur.pb.b64.bz2 line file, or
    train_it = device_batches(index, other, count, batch_size)  # straight into train_epoch, no file

Semantics (make_dice.py:41-54): with u = the sorted distinct ids of a document, every i < j adds 1 to the entry
(index = u[i], other = u[j]) -- ``index < other``, the opposite orientation to the windowed matrix.  The sums are uint64
(esr_dice.hip), so the result does not depend on atomic order, on how documents are cut into ``add`` calls or on how an
``add`` is cut into launches; ``count = float32(sum)``.

The one deviation from the reference: a document holds at most ``MAX_DOC`` = 4096 ids, repeats counted (the kernel sorts
a document in LDS).  A longer document raises ``ValueError`` on the host, before any launch; it is never truncated.

Document frequency is build-defined: the reference reads ``doc_frequency`` from its dictionary file, which is made
elsewhere; here the builder counts it in the same pass -- ``df[id]`` = the number of documents whose set contains ``id``.
"""
import types

import numpy as np
import torch

from .. import ops
from .make_cooccurrence import device_batches, pack_docs, split_rows, write_cooccurrence  # noqa: F401 (re-exported)
from .pair_table import (FAILURES as TABLE_FAILURES, CooccurrenceError, PairTable, csr_inputs, host_offsets,  # noqa: F401
                         plan_ranges, pow2_at_least)

# Flags with the reference's names and defaults (make_dice.py:19-22).  input_file is an .npz of `indices` / `doc_offsets`.
FLAGS = types.SimpleNamespace(input_file=None, output_file=None, max_row_size=1000)

MAX_DOC = 4096   # esr_dice_max_doc(): ids per document, repeats counted
FAILURES = dict(TABLE_FAILURES)
FAILURES[2] = "a negative id"
FAILURES[4] = "doc_offsets outside [0, N] (or overlapping documents)"
FAILURES[16] = "a document above %d ids" % MAX_DOC


def check_doc_sizes(doc_offsets, max_doc=MAX_DOC):
    """Raises ValueError naming the first document of more than max_doc ids.  Host work on doc_offsets alone."""
    n = np.diff(host_offsets(doc_offsets))
    long_ = np.flatnonzero(n > max_doc)
    if long_.size:
        d = int(long_[0])
        raise ValueError("document %d holds %d ids, above the cap of %d ids per document (esr_dice.hip sorts a document "
                         "in LDS); split or sample it before add" % (d, int(n[d]), max_doc))


def pair_bounds(doc_offsets):
    """Per document, what it can add to the table at most: n (n - 1) / 2 pair keys + n diagonal keys (n = its length)."""
    n = np.diff(host_offsets(doc_offsets))
    return n * (n - 1) // 2 + n


def plan_launches(doc_offsets, max_pairs_per_launch):
    """[(doc_begin, doc_end, bound), ...]: consecutive document ranges that cover every document exactly once, each with
    bound = the sum of its documents' pair_bounds <= max_pairs_per_launch -- or holding ONE document, when that document's
    own bound is above the limit (a document is never cut)."""
    return plan_ranges(np.concatenate([[0], np.cumsum(pair_bounds(doc_offsets))]), max_pairs_per_launch)


class DiceBuilder:
    """Reduce-by-key of the set pairs of a corpus in the device hash table of ``CooccurrenceBuilder`` (open addressing,
    64-bit keys ``index << 32 | other``, uint64 counts).  The document frequencies live in the same table on the diagonal
    keys ``id << 32 | id``, which no pair can make; ``finalize`` and ``doc_frequency`` split them off.

    Growth rule (``PairTable``): the host computes ``sum of n (n - 1) / 2 + n`` per document range from ``doc_offsets``
    and cuts an ``add`` into ranges whose bound is at most ``max_pairs_per_launch`` (``plan_launches``); that bound is
    reserved before the launch.

    A failure word raised by the device (a negative id in a device tensor, broken offsets) becomes a ``CooccurrenceError``
    and leaves the builder unusable, as in ``CooccurrenceBuilder``."""

    def __init__(self, capacity=1 << 20, device=None, max_pairs_per_launch=1 << 26):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_pairs_per_launch = max(int(max_pairs_per_launch), 1)
        self.launches = 0
        self._max_id = -1
        self._pairs = PairTable(capacity, self.device, FAILURES)
        self._result = None     # (index, other, count, ids, df) of the table as it stands

    capacity = property(lambda self: self._pairs.capacity)
    rehashes = property(lambda self: self._pairs.rehashes)

    def add(self, indices, doc_offsets):
        """Adds the documents ``indices[doc_offsets[d]:doc_offsets[d + 1]]`` (numpy arrays or device tensors)."""
        pairs = self._pairs
        pairs.check_usable()
        off_host = host_offsets(doc_offsets)
        check_doc_sizes(off_host)
        indices, off_host, off_dev = csr_inputs(indices, doc_offsets, self.device, "indices", off_host)
        if indices.numel() == 0 or off_host.size == 1:
            return self
        with torch.cuda.device(self.device):
            ws = ops.dice_workspace(indices.numel(), self.device)
            self._result = None
            for a, b, bound in plan_launches(off_host, self.max_pairs_per_launch):
                if bound == 0:
                    continue
                pairs.reserve(bound)
                ops.dice_accumulate(pairs.tensor, pairs.capacity, indices, off_dev, a, b, ws)
                self.launches += 1
                pairs.sync()
                pairs.settle()
            self._max_id = max(self._max_id, int(indices.max()))
        return self

    def _finalized(self):
        self._pairs.check_usable()
        if self._result is None:
            with torch.cuda.device(self.device):
                index, other, count = self._pairs.finalize(self._max_id + 1)
                diag = index == other
                pair = ~diag
                self._result = (index[pair], other[pair], count[pair], index[diag], count[diag])
        return self._result

    @property
    def nnz(self):
        """Distinct (index, other) pairs so far (the table's occupied slots without the diagonal ones)."""
        return int(self._finalized()[0].numel())

    def finalize(self):
        """(index int32[nnz], other int32[nnz], count float32[nnz]) on the device, ascending by (index, other), with
        index < other.  The builder stays usable: more ``add`` calls may follow."""
        return self._finalized()[:3]

    def doc_frequency(self):
        """(ids int32[u], df float32[u]) on the device, ascending by id: df = the number of documents added so far whose
        set contains the id.  Build-defined: the reference reads these from its dictionary file."""
        return self._finalized()[3:]


def process_sdocs(docs, device=None):
    """``process_sdoc`` over every document plus the reduce (make_dice.py:41-54, 97-98): an iterable of id lists (primary
    index first, then the secondary indices) -> (index, other, count) device tensors ascending by (index, other)."""
    indices, offsets = pack_docs(docs)
    bound = int(pair_bounds(offsets).sum())
    builder = DiceBuilder(capacity=pow2_at_least(min(1 << 20, 2 * max(1, bound))), device=device)
    return builder.add(indices, offsets).finalize()


def dice_scores(index, other, count, ids, df):
    """dump_dice.py:36-45: ``joint_count / (doc_frequency[other] + doc_frequency[index])`` per entry -- without the factor
    2 of the textbook Dice coefficient, as the reference has it.  (ids, df) as ``doc_frequency`` returns them (ids
    ascending).  float32[nnz], plain torch."""
    ids = ids.to(torch.int64)
    df = df.to(torch.float32)
    pos_i = torch.searchsorted(ids, index.to(torch.int64))
    pos_o = torch.searchsorted(ids, other.to(torch.int64))
    return count.to(torch.float32) / (df[pos_o] + df[pos_i])


def main(argv=None):
    """input_file: an .npz of `indices` / `doc_offsets`; output_file: the cooccur.pb.b64.bz2 file."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input_file", required=True, help="Input .npz of indices / doc_offsets.")
    ap.add_argument("--output_file", required=True, help="Output cooccur.pb.b64.bz2 file.")
    ap.add_argument("--max_row_size", type=int, default=FLAGS.max_row_size, help="Max number of items per row.")
    args = ap.parse_args(argv)
    with np.load(args.input_file) as z:
        indices, doc_offsets = z["indices"], z["doc_offsets"]
    builder = DiceBuilder()
    index, other, count = builder.add(indices, doc_offsets).finalize()
    lines = write_cooccurrence(args.output_file, index, other, count, args.max_row_size)
    print("wrote %d pairs in %d rows to %s" % (builder.nnz, lines, args.output_file))


if __name__ == "__main__":
    main()

"""What the corpus-to-matrix builders share (``make_cooccurrence``, ``make_dice``, ``make_dictionary``, ``count_terms``): they
all reduce by key into the open-addressing pair table of esr_cooccur_table.h.  Here is the table's owner with its growth
rule (``PairTable``), the check of CSR inputs (``csr_inputs``) and the cut of an ``add`` into launches (``plan_ranges``).
"""
import numpy as np
import torch

from .. import ops

# the failure word of the table's header, bit -> text; a builder passes its own wording where its kernels mean another thing
FAILURES = {1: "a probe wrapped the whole table (capacity below occupied + emitted pairs)", 2: "a negative token id",
            4: "doc_offsets outside [0, N]", 8: "finalize: nnz below the table's occupied count"}


class CooccurrenceError(RuntimeError):
    """The device raised the table's failure word; the builder that saw it is unusable."""


def pow2_at_least(n):
    c = 2
    while c < n:
        c <<= 1
    return c


def failure_text(fail, failures):
    return "; ".join(msg for bit, msg in failures.items() if fail & bit)


class PairTable:
    """One pair table on `device`: the tensor, its ``capacity`` (a power of two), the occupied slots ``used`` as of the
    last ``sync``, the ``rehashes`` so far and the failed state.  The table is made at the first ``reserve``, so an owner
    that refuses its input on the host touches no device.

    Growth rule -- a correctness condition, not tuning: a probe must find its key or an empty slot, so before a launch
    ``reserve(extra)`` makes ``capacity >= used + extra`` with extra = the keys the launch can emit at most; after it,
    ``sync`` reads the header (one host sync per launch: this is ETL) and ``settle`` doubles the table until its load
    factor is at most 1/2.  Growing re-inserts the occupied slots into a new table (esr_cooccur_rehash).

    A failure word raised by the device becomes a ``CooccurrenceError`` that starts with `what` and spells the bits with
    `failures`; from then on every call raises.

    `table_ops` = (make(capacity, device), rehash(tensor, capacity, new_capacity)) of a table with another slot layout
    behind the same 256-byte header (the wide table of ``ratings``); the default is the narrow table's."""

    def __init__(self, capacity, device, failures=FAILURES, what="co-occurrence table", tensor=None, table_ops=None):
        self.capacity = pow2_at_least(int(capacity))
        self.device, self.failures, self.what = device, failures, what
        self.tensor = tensor        # given: a table that a kernel filled whole (the dictionary lookup)
        self.used = 0
        self.rehashes = 0
        self.failed = None
        self._make, self._rehash = table_ops if table_ops is not None else (ops.cooccur_table, ops.cooccur_rehash)

    def check_usable(self):
        if self.failed is not None:
            raise CooccurrenceError("this builder is unusable: " + self.failed)

    def _grow_to(self, capacity):
        self.check_usable()
        if self.tensor is None:
            self.capacity = max(self.capacity, capacity)
            self.tensor = self._make(self.capacity, self.device)
        elif capacity > self.capacity:
            self.tensor = self._rehash(self.tensor, self.capacity, capacity)
            self.capacity = capacity
            self.rehashes += 1

    def reserve(self, extra):
        """Room for `extra` more keys, whatever the table holds: made now, or rehashed when it is too small."""
        self._grow_to(pow2_at_least(self.used + int(extra)))
        return self

    def header(self):
        """(occupied slots, failure bits) as the device has them: a sync."""
        return ops.cooccur_header(self.tensor)

    def sync(self):
        """Reads the header: ``used``, or ``CooccurrenceError`` and a table that stays unusable."""
        self.check_usable()
        used, fail = self.header()
        if fail:
            self.failed = failure_text(fail, self.failures)
            raise CooccurrenceError("%s failure (bits %d): %s" % (self.what, fail, self.failed))
        self.used = used
        return used

    def settle(self):
        """After a launch and its ``sync``: doubles the table until its load factor is at most 1/2."""
        self.check_usable()
        while 2 * self.used > self.capacity:
            self._grow_to(2 * self.capacity)

    def finalize(self, num_ids, context_window=1):
        """(index, other, count) of every occupied slot, ascending by (index, other) (esr_cooccur_finalize); empty device
        tensors from a table that holds nothing, made or not."""
        self.check_usable()
        if not self.used:
            return (torch.empty(0, dtype=torch.int32, device=self.device), torch.empty(0, dtype=torch.int32, device=self.device),
                    torch.empty(0, dtype=torch.float32, device=self.device))
        out = ops.cooccur_finalize(self.tensor, self.capacity, self.used, num_ids, context_window)
        self.sync()
        return out


def host_offsets(doc_offsets, n=None, what="tokens"):
    """doc_offsets as a host int64 array, checked: one dimension and, with `n`, rising from 0 to n.  ValueError
    otherwise -- before any launch."""
    off = doc_offsets.cpu().numpy() if isinstance(doc_offsets, torch.Tensor) else np.asarray(doc_offsets)
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError("doc_offsets must be int64 [ndocs + 1]")
    if n is not None and (off[0] != 0 or off[-1] != n or (off.size > 1 and np.any(np.diff(off) < 0))):
        raise ValueError("doc_offsets must rise from 0 to len(%s) = %d" % (what, n))
    return off


def csr_inputs(ids, doc_offsets, device, what, off_host=None):
    """(ids int32[N] on `device`, offsets host, offsets on `device`) of the documents ``ids[doc_offsets[d]:doc_offsets[d +
    1]]`` (numpy arrays or tensors), with every host-side check done before the device is touched.  `what` names the ids in
    the message; `off_host` is ``host_offsets(doc_offsets)`` from a caller that had to look at the offsets first.  Ids are
    not screened here: the kernels do that (failure bit 2)."""
    n = ids.numel() if isinstance(ids, torch.Tensor) else np.asarray(ids).size
    off_host = host_offsets(doc_offsets if off_host is None else off_host, n, what)
    ids = ops.as_ids(ids.to(device) if isinstance(ids, torch.Tensor) else ids, device).reshape(-1)
    if isinstance(doc_offsets, torch.Tensor) and doc_offsets.is_cuda and doc_offsets.dtype == torch.int64 and \
            doc_offsets.is_contiguous() and doc_offsets.device == ids.device:
        off_dev = doc_offsets
    else:
        off_dev = torch.from_numpy(off_host).to(device)
    return ids, off_host, off_dev


def plan_ranges(cumulative, limit):
    """[(begin, end, cost), ...]: consecutive ranges that cover the items [0, len(cumulative) - 1) exactly once, each with
    cost = cumulative[end] - cumulative[begin] <= limit -- or holding ONE item, when that item alone costs more (an item,
    a document, is never cut)."""
    cum = np.asarray(cumulative, dtype=np.int64)
    limit = max(int(limit), 1)
    n = cum.size - 1
    plan = []
    a = 0
    while a < n:
        b = int(np.searchsorted(cum, cum[a] + limit, side="right")) - 1   # the last b with cum[b] - cum[a] <= limit
        b = min(max(b, a + 1), n)
        plan.append((a, b, int(cum[b] - cum[a])))
        a = b
    return plan

"""Makes the co-occurrence matrix -- the step in front of the GloVe trainer (the reference's
``wikipedia/make_cooccurrence.py``, a PySpark job there) on the GPU, from token-id streams.

Tokenising is host string work and stays outside; the token -> embedding-index dictionary is made on the GPU from
provisional ids by ``make_dictionary`` (``TermStatsBuilder``, ``make_token_dictionary``, ``Dictionary.embedding_indices``),
whose output is this module's input: ``tokens int32[N]`` with ``doc_offsets int64[ndocs + 1]`` (CSR; document d is
``tokens[doc_offsets[d]:doc_offsets[d + 1]]``).

    builder = CooccurrenceBuilder(context_window=10)
    builder.add(tokens, doc_offsets)            # any number of times: the reduce-by-key over the corpus
    index, other, count = builder.finalize()    # device tensors, ascending by (index, other)
    write_cooccurrence(path, index, other, count)               # the reference's *.cooccur.pb.b64.bz2 line file, or
    train_it = device_batches(index, other, count, batch_size)  # straight into train_epoch, no file

Semantics (make_cooccurrence.py:33-55): position i pairs with j in ``range(max(0, i - W), min(n, i + W))`` -- W back, W - 1
forward -- and adds ``1 / |i - j|`` to entry (t[i], t[j]) when t[i] > t[j].  The sums are kept in fixed point (units of
1 / lcm(1..W), uint64: esr_cooccur.hip), so the result does not depend on atomic order or on how the corpus is cut into
``add`` calls; ``count = float32(float64(sum) / lcm)``.
"""
import types

import numpy as np
import torch

from .. import ops
from .pair_table import CooccurrenceError, PairTable, csr_inputs, pow2_at_least  # noqa: F401 (CooccurrenceError: re-exported)
from .wire import packed_varints, varint, write_lines

# Flags with the reference's names and defaults (make_cooccurrence.py:23-27; token_dictionary has no part here: ids come
# in).  input_file is an .npz of `tokens` / `doc_offsets`.
FLAGS = types.SimpleNamespace(input_file=None, output_file=None, context_window=10, max_row_size=1000)

MAX_CONTEXT_WINDOW = 22   # lcm(1..22) < 2^28: 2^36 window hits fit a uint64 sum


class CooccurrenceBuilder:
    """Reduce-by-key of the window pairs of a corpus in a device hash table (open addressing, 64-bit keys
    ``index << 32 | other``, uint64 fixed-point sums).

    Growth rule (``PairTable``): a launch covers a token range of at most ``max_pairs_per_launch / context_window``
    positions, each of which emits at most context_window pairs -- that many keys are reserved before it.  The table is
    made at the first launch."""

    def __init__(self, context_window=10, capacity=1 << 20, device=None, max_pairs_per_launch=1 << 26):
        if not 1 <= int(context_window) <= MAX_CONTEXT_WINDOW:
            raise ValueError("context_window must be in [1, %d], got %r" % (MAX_CONTEXT_WINDOW, context_window))
        self.context_window = int(context_window)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_pairs_per_launch = max(int(max_pairs_per_launch), self.context_window)
        self._max_id = -1
        self._pairs = PairTable(capacity, self.device)

    capacity = property(lambda self: self._pairs.capacity)
    rehashes = property(lambda self: self._pairs.rehashes)
    nnz = property(lambda self: self._pairs.used, doc="Distinct (index, other) pairs so far.")

    def add(self, tokens, doc_offsets):
        """Adds the documents ``tokens[doc_offsets[d]:doc_offsets[d + 1]]`` (numpy arrays or device tensors)."""
        pairs, W = self._pairs, self.context_window
        pairs.check_usable()
        tokens, off_host, off_dev = csr_inputs(tokens, doc_offsets, self.device, "tokens")
        N = tokens.numel()
        if N == 0 or off_host.size == 1:
            return self
        with torch.cuda.device(self.device):
            step = max(1, self.max_pairs_per_launch // W)
            for a in range(0, N, step):
                b = min(N, a + step)
                pairs.reserve((b - a) * W)
                ops.cooccur_accumulate(pairs.tensor, pairs.capacity, tokens, off_dev, a, b, W)
                pairs.sync()
                pairs.settle()
            self._max_id = max(self._max_id, int(tokens.max()))
        return self

    def finalize(self):
        """(index int32[nnz], other int32[nnz], count float32[nnz]) on the device, ascending by (index, other).  The
        builder stays usable: more ``add`` calls may follow."""
        with torch.cuda.device(self.device):
            return self._pairs.finalize(self._max_id + 1, self.context_window)


def pack_docs(docs):
    """An iterable of id lists -> (tokens int32[N], doc_offsets int64[ndocs + 1])."""
    docs = [np.asarray(d, dtype=np.int32).reshape(-1) for d in docs]
    offsets = np.zeros(len(docs) + 1, np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=offsets[1:])
    tokens = np.concatenate(docs) if docs else np.zeros(0, np.int32)
    return tokens.astype(np.int32, copy=False), offsets


def process_docs(docs, context_window=10, device=None):
    """``process_doc`` over every document plus the reduce (make_cooccurrence.py:33-55, 95-96): an iterable of embedding
    index lists -> (index, other, count) device tensors ascending by (index, other)."""
    tokens, offsets = pack_docs(docs)
    builder = CooccurrenceBuilder(context_window, capacity=pow2_at_least(min(1 << 20, 2 * max(1, tokens.size))),
                                  device=device)
    return builder.add(tokens, offsets).finalize()


def encode_cooccurrence_row(index, others, counts):
    """One ``CooccurrenceRow`` (proto/nlp.proto: uint64 index = 1; repeated uint64 other_index = 2; repeated float
    count = 3) as protobuf's proto3 serialiser writes it: field 1 a varint (left out when zero), fields 2 and 3 packed
    (left out when empty)."""
    out = bytearray()
    if index:
        out += b"\x08" + varint(int(index))
    if len(others):
        body = packed_varints(others)
        out += b"\x12" + varint(len(body)) + body
    if len(counts):
        body = np.asarray(counts, dtype="<f4").tobytes()
        out += b"\x1a" + varint(len(body)) + body
    return bytes(out)


def split_rows(index, max_row_size=1000):
    """[(start, end), ...] of the row pieces of an index-grouped entry list: a piece ends at a change of index, or once it
    holds MORE than max_row_size entries (``len(proto.count) > max_row_size`` after an append: full pieces hold
    max_row_size + 1 -- the reference's own off-by-one, make_cooccurrence.py:87)."""
    index = np.asarray(index)
    n = index.size
    if n == 0:
        return []
    bounds = np.flatnonzero(np.diff(index)) + 1
    pieces = []
    full = int(max_row_size) + 1
    for a, b in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [n]])):
        for s in range(a, b, full):
            pieces.append((int(s), int(min(b, s + full))))
    return pieces


def write_cooccurrence(path, index, other, count, max_row_size=1000):
    """Writes (index, other, count) -- grouped by index, as ``finalize`` returns them -- as a ``*.cooccur.pb.b64.bz2``
    line file: one base64 ``CooccurrenceRow`` per line, bz2 (make_cooccurrence.py:80-100).  Returns the line count."""
    index, other, count = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (index, other, count))
    return write_lines(path, (encode_cooccurrence_row(index[a], other[a:b], count[a:b])
                              for a, b in split_rows(index, max_row_size)))


def device_batches(index, other, count, batch_size, generator=None):
    """Batches ``(int32[2, B], float32[B])`` of the finalized matrix as device tensors, forever (as ``get_batch`` cycles
    over its files): one ``torch.randperm`` per pass, every entry exactly once per pass, a batch may straddle two passes.
    Usable as ``train_it`` of ``train_epoch`` -- device id tensors pass through ``ops.as_ids`` untouched -- so training
    needs no file."""
    nnz = index.numel()
    if nnz == 0:
        raise ValueError("device_batches: the matrix is empty")
    B = int(batch_size)
    pairs = torch.stack([index, other]).to(torch.int32)
    count = count.to(torch.float32)
    order = torch.randperm(nnz, device=index.device, generator=generator)
    pos = 0
    while True:
        take = [order[pos:pos + B]]
        pos += B
        while pos > nnz:
            order = torch.randperm(nnz, device=index.device, generator=generator)
            pos -= nnz
            take.append(order[:pos] if pos <= nnz else order)
        sel = take[0] if len(take) == 1 else torch.cat(take)
        yield pairs[:, sel].contiguous(), count[sel].contiguous()


def main(argv=None):
    """input_file: an .npz of `tokens` / `doc_offsets`; output_file: the cooccur.pb.b64.bz2 file."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input_file", required=True, help="Input .npz of tokens / doc_offsets.")
    ap.add_argument("--output_file", required=True, help="Output cooccur.pb.b64.bz2 file.")
    ap.add_argument("--context_window", type=int, default=FLAGS.context_window, help="Size of the context window.")
    ap.add_argument("--max_row_size", type=int, default=FLAGS.max_row_size, help="Max number of items per row.")
    args = ap.parse_args(argv)
    with np.load(args.input_file) as z:
        tokens, doc_offsets = z["tokens"], z["doc_offsets"]
    builder = CooccurrenceBuilder(args.context_window)
    index, other, count = builder.add(tokens, doc_offsets).finalize()
    lines = write_cooccurrence(args.output_file, index, other, count, args.max_row_size)
    print("wrote %d pairs in %d rows to %s" % (builder.nnz, lines, args.output_file))


if __name__ == "__main__":
    main()

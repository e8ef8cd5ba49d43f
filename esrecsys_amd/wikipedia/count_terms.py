"""Makes tf-idf sparse documents -- ``make_sparse_doc`` of the reference's ``wikipedia/count_terms.py:32-74`` (a Python
loop per document there) -- on the GPU, from provisional token ids and a ``make_dictionary.Dictionary``.

    builder = TfidfBuilder(dictionary, stopwords={raw ids})
    out_offsets, token_index, token_tfidf = builder.transform(tokens, doc_offsets)   # device tensors, CSR
    write_sparse_docs(path, primary_index, out_offsets, token_index, token_tfidf)    # SparseDocument line file

Semantics: document d's row holds the distinct dictionary indices of its tokens -- stopwords (raw ids) skipped before
counting, tokens outside the dictionary dropped, tf counting every occurrence.  In fp64, as the reference's Python floats:
``idf = max(0, log1p(max_doc_frequency) - log1p(df) + 1)``, ``tfidf = tf * idf``, ``norm = sum tfidf^2``,
``tfidf *= 1 / sqrt(norm)`` (0 where ``norm == 0``), stored as float32.  The idf table (one entry per dictionary index) is
computed on the host with NumPy in fp64 exactly as written; the device does the rest in fp64 and rounds to float32 at
the store.  Empty documents, and documents with no dictionary token, give empty rows.

Stated deviation from the reference: a row is ordered by ascending index; the reference's order is dict insertion order,
that is, first occurrence.  The norm is then summed in that order -- lane-strided over the sorted row and by a fixed
butterfly across one wave (esr_terms.hip), so two runs give the same bits; against the reference's order the fp64 sum of n
squares differs by at most about n 2^-53 relative, which can move the float32 rounding only at a tie.

Only the token part of ``SparseDocument`` is made here: ``primary_index`` is the caller's (a title-dictionary lookup,
``Dictionary.index_of`` of the title ids), the secondary titles and the url are left out.
"""
import numpy as np
import torch

from .. import ops
from .make_dictionary import FAILURES, plan_launches, token_inputs
from .pair_table import PairTable
from .wire import packed_varints, varint, write_lines


def idf_table(doc_frequency, max_doc_frequency):
    """float64[K], count_terms.py:58-62 and 78-79 as written: ``log1p(max_doc_frequency) - log1p(df) + 1.0``, clamped at 0."""
    df = doc_frequency.cpu().numpy() if isinstance(doc_frequency, torch.Tensor) else np.asarray(doc_frequency)
    idf = np.log1p(np.float64(max_doc_frequency)) - np.log1p(df.astype(np.float64)) + 1.0
    idf[idf < 0.0] = 0.0
    return idf


class TfidfBuilder:
    """``make_sparse_doc`` over CSR token documents.  Per launch (whole documents, ``make_dictionary.plan_launches``; a
    document longer than ``max_tokens_per_launch`` is its own launch): the accumulate kernel of ``TermStatsBuilder``,
    here with the dictionary's lookup table (stopwords left out of it), reduces the tokens into a scratch pair table
    keyed ``document in launch << 32 | index`` holding tf; the table's compact and two-pass sort (esr_cooccur_finalize)
    order the keys by (document, index); esr_run_offsets cuts them into rows; one kernel scales and normalises the rows.
    Nothing depends on atomic order or on ``max_tokens_per_launch``.

    A failure word raised by the device becomes a ``CooccurrenceError`` and leaves the builder unusable."""

    def __init__(self, dictionary, stopwords=None, device=None, max_tokens_per_launch=1 << 21):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dictionary = dictionary
        self.stopwords = frozenset(int(s) for s in stopwords) if stopwords else frozenset()
        self.max_tokens_per_launch = max(int(max_tokens_per_launch), 1)
        self.launches = 0
        self._scratch = self._new_scratch()   # the last launch's: it holds the failed state
        self._lookup = None     # made at the first launch: a refused transform touches no device
        self._idf = None

    def _new_scratch(self):
        return PairTable(2, self.device, FAILURES, "tf-idf scratch table")

    def _prepare(self):
        if self._lookup is None:
            self._lookup = self.dictionary.lookup_table(self.device, skip=self.stopwords or None)
            self._idf = torch.from_numpy(idf_table(self.dictionary.doc_frequency, self.dictionary.max_doc_frequency)) \
                .to(self.device)

    def transform(self, tokens, doc_offsets):
        """(out_offsets int64[ndocs + 1], token_index int32[nnz], token_tfidf float32[nnz]) on the device: row d is
        ``[out_offsets[d], out_offsets[d + 1])``, ascending by index."""
        self._scratch.check_usable()
        tokens, off_host, off_dev = token_inputs(tokens, doc_offsets, self.device)
        with torch.cuda.device(self.device):
            ndocs = off_host.size - 1
            K = self.dictionary.size
            pieces_off = [torch.zeros(1, dtype=torch.int64, device=self.device)]
            pieces_index, pieces_tfidf = [], []
            base = 0
            for a, b, n in plan_launches(off_host, self.max_tokens_per_launch) if ndocs and K else []:
                rows = b - a
                used = 0
                if n:
                    self._prepare()
                    lookup, lookup_capacity = self._lookup
                    self._scratch = self._new_scratch().reserve(2 * n)
                    scratch, capacity = self._scratch.tensor, self._scratch.capacity
                    ops.terms_accumulate(scratch, capacity, tokens, off_dev, a, b, int(off_host[a]), int(off_host[b]),
                                         lookup, lookup_capacity)
                    self.launches += 1
                    used = self._scratch.sync()
                if used == 0:
                    pieces_off.append(torch.full((rows,), base, dtype=torch.int64, device=self.device))
                    continue
                doc, index, _ = ops.cooccur_finalize(scratch, capacity, used, max(rows, K), 1)   # _ = float32(tf): unused
                row_off = ops.run_offsets(doc, rows)
                pieces_tfidf.append(ops.terms_tfidf_rows(scratch, capacity, index, row_off, self._idf))
                pieces_index.append(index)
                pieces_off.append(row_off[1:].to(torch.int64) + base)
                base += used
            if not (ndocs and K):
                pieces_off.append(torch.zeros(ndocs, dtype=torch.int64, device=self.device))
            out_offsets = torch.cat(pieces_off)
            if pieces_index:
                return out_offsets, torch.cat(pieces_index), torch.cat(pieces_tfidf)
            return out_offsets, torch.empty(0, dtype=torch.int32, device=self.device), \
                torch.empty(0, dtype=torch.float32, device=self.device)


# ---- the SparseDocument line file (proto/nlp.proto:34-41: uint64 primary_index = 2; repeated uint64 token_index = 4;
# repeated float token_tfidf = 5) ----
def encode_sparse_document(primary_index, token_index, token_tfidf):
    """One ``SparseDocument`` as protobuf's proto3 serialiser writes it: field 2 a varint (left out when zero), fields 4
    and 5 packed (left out when empty)."""
    out = bytearray()
    if primary_index:
        out += b"\x10" + varint(int(primary_index))
    if len(token_index):
        body = packed_varints(token_index)
        out += b"\x22" + varint(len(body)) + body
    if len(token_tfidf):
        body = np.asarray(token_tfidf, dtype="<f4").tobytes()
        out += b"\x2a" + varint(len(body)) + body
    return bytes(out)


def write_sparse_docs(path, primary_index, out_offsets, token_index, token_tfidf):
    """Writes one base64 ``SparseDocument`` per document, bz2 (the reference's ``sparse.pb.b64.bz2``): ``primary_index``
    holds one title index per document (None: all left out), the rest is what ``transform`` returns.  Returns the line
    count."""
    out_offsets, token_index, token_tfidf = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
                                             for x in (out_offsets, token_index, token_tfidf))
    ndocs = out_offsets.size - 1
    if primary_index is None:
        primary_index = np.zeros(ndocs, np.int64)
    primary_index = primary_index.cpu().numpy() if isinstance(primary_index, torch.Tensor) else np.asarray(primary_index)
    if primary_index.size != ndocs:
        raise ValueError("primary_index must hold one index per document: %d for %d" % (primary_index.size, ndocs))
    return write_lines(path, (encode_sparse_document(primary_index[d], token_index[out_offsets[d]:out_offsets[d + 1]],
                                                     token_tfidf[out_offsets[d]:out_offsets[d + 1]]) for d in range(ndocs)))

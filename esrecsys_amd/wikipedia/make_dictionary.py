"""Makes the token dictionary -- the reference's ``wikipedia/make_dictionary.py`` (a PySpark job there) and the lookup of
``wikipedia/token_dictionary.py`` -- on the GPU, from provisional token ids.

What the host decides is only the strings: interning a string to a provisional int is one dict lookup.  The input is
``tokens int32[N] >= 0`` (provisional ids: any values up to 2^31 - 1, not dense) with ``doc_offsets int64[ndocs + 1]``
(CSR, as ``CooccurrenceBuilder.add`` takes it; numpy arrays or device tensors).

    stats = TermStatsBuilder()
    stats.add(tokens, doc_offsets)                       # any number of times
    ids, frequency, doc_frequency = stats.finalize()     # device tensors, ascending by id
    dictionary = make_token_dictionary(ids, frequency, doc_frequency)
    indices = dictionary.embedding_indices(tokens)       # what CooccurrenceBuilder.add takes
    write_dictionary(path, dictionary, token_of)         # the reference's TokenStat line file

Semantics: ``frequency[id]`` = occurrences, ``doc_frequency[id]`` = documents that hold the id at least once
(make_dictionary.py:67-74, 101-105); keep ``frequency >= min_frequency``, sort by frequency descending, keep the first
``min(max_size, count)``, the position is the index (make_dictionary.py:108-117); embedding index = ``1 + index`` inside the
dictionary, ``1 + size + bucket`` outside, embedding size = ``1 + 65536 + size`` (token_dictionary.py:58-68).

Stated deviations from the reference:
  tie order   the reference breaks frequency ties by Spark's ``collect()`` order, which is unspecified; here ties go by
              ascending id.
  OOV bucket  the reference's ``minhash`` is a function of the token's STRING, so it is host work: the caller supplies it
              per token as ``oov_bucket int32[N]`` in ``[0, 65536)``; without one the bucket is ``raw id & 0xFFFF``.

All counts are uint64 sums in the pair table of ``CooccurrenceBuilder`` (esr_terms.hip): results do not depend on atomic
order, on how the corpus is cut into ``add`` calls or on ``max_tokens_per_launch``.
"""
import base64
import bz2
import types

import numpy as np
import torch

from .. import ops
from . import pair_table
from .pair_table import FAILURES as TABLE_FAILURES, PairTable, csr_inputs, failure_text, plan_ranges, pow2_at_least
from .wire import read_varint, varint, write_lines

# Flags with the reference's names and defaults (make_dictionary.py:19-31; the title dictionary is the same job over the
# titles: call the same functions with the title flags).  input_file is an .npz of `tokens` / `doc_offsets`.
FLAGS = types.SimpleNamespace(input_file=None, token_output=None, title_output=None, min_token_frequency=20,
                              max_token_dictionary_size=500000, max_title_dictionary_size=500000, min_title_frequency=5)

OOV_BUCKETS = 65536
FAILURES = dict(TABLE_FAILURES)
FAILURES[2] = "a negative id"
FAILURES[4] = "doc_offsets on the device differ from the host's plan"
FAILURES[32] = "an oov_bucket outside [0, %d)" % OOV_BUCKETS


# ---- host-side argument checks and launch planning (no device) ----
def host_offsets(doc_offsets, n_tokens):
    """doc_offsets as a host int64 array, checked: one dimension, rising from 0 to n_tokens.  ValueError otherwise --
    before any launch."""
    return pair_table.host_offsets(doc_offsets, n_tokens)


def check_host_tokens(tokens):
    """A host token array (numpy / list) as int32, ValueError on a negative id or one above 2^31 - 1.  Device tensors are
    screened by the kernels (failure bit 2)."""
    a = np.asarray(tokens)
    if a.size and (a.min() < 0 or a.max() > 2 ** 31 - 1):
        raise ValueError("token ids must be in [0, 2^31 - 1]: min %d max %d" % (a.min(), a.max()))
    return np.array(a, dtype=np.int32).reshape(-1)     # (a copy: the caller's array may be read-only)


def check_host_buckets(oov_bucket, n_tokens):
    """A host oov_bucket array as int32, ValueError unless it has one value in [0, 65536) per token."""
    a = np.asarray(oov_bucket)
    if a.size != n_tokens:
        raise ValueError("oov_bucket must hold one bucket per token: %d for %d tokens" % (a.size, n_tokens))
    if a.size and (a.min() < 0 or a.max() >= OOV_BUCKETS):
        raise ValueError("oov_bucket must be in [0, %d): min %d max %d" % (OOV_BUCKETS, a.min(), a.max()))
    return np.array(a, dtype=np.int32).reshape(-1)     # (a copy: the caller's array may be read-only)


def plan_launches(doc_offsets, max_tokens_per_launch):
    """[(doc_begin, doc_end, tokens), ...]: consecutive document ranges that cover every document exactly once, each of
    at most max_tokens_per_launch tokens -- or holding ONE document, when that document alone is longer (a document is
    never cut, and there is no cap on its length)."""
    return plan_ranges(doc_offsets, max_tokens_per_launch)


def token_inputs(tokens, doc_offsets, device):
    """``csr_inputs`` behind the terms builders' host screen: a host token array goes through ``check_host_tokens``."""
    return csr_inputs(tokens if isinstance(tokens, torch.Tensor) else check_host_tokens(tokens), doc_offsets, device,
                      "tokens")


class TermStatsBuilder:
    """``count_tokens`` over a corpus plus ``tokenstat_reducer`` (make_dictionary.py:67-74, 101-105).

    A launch covers whole documents (``plan_launches``; a document longer than ``max_tokens_per_launch`` is its own
    launch).  Its tokens are reduced into a scratch pair table keyed ``document in launch << 32 | id`` -- equal keys of a
    wave merged before the atomic -- and a second kernel folds every occupied scratch slot into the persistent table:
    ``id << 32 | 0`` += tf, ``id << 32 | 1`` += 1.  Contention on a hot id is per document, not per occurrence, and
    nothing persistent grows with the number of documents.

    Growth rule (``PairTable``): a launch of n tokens reserves 2 n keys in its scratch table and 2 n more in the
    persistent one.

    A failure word raised by the device (a negative id in a device tensor, offsets that differ) becomes a
    ``CooccurrenceError`` and leaves the builder unusable, as in ``CooccurrenceBuilder``."""

    def __init__(self, capacity=1 << 20, device=None, max_tokens_per_launch=1 << 21):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_tokens_per_launch = max(int(max_tokens_per_launch), 1)
        self.launches = 0
        self._pairs = PairTable(capacity, self.device, FAILURES, "term statistics table")
        self._result = None

    capacity = property(lambda self: self._pairs.capacity)
    rehashes = property(lambda self: self._pairs.rehashes)
    num_ids = property(lambda self: self._pairs.used // 2, doc="Distinct ids so far (every id holds two slots of the table).")

    def add(self, tokens, doc_offsets):
        """Adds the documents ``tokens[doc_offsets[d]:doc_offsets[d + 1]]`` (numpy arrays or device tensors)."""
        pairs = self._pairs
        pairs.check_usable()
        tokens, off_host, off_dev = token_inputs(tokens, doc_offsets, self.device)
        if tokens.numel() == 0 or off_host.size == 1:
            return self
        with torch.cuda.device(self.device):
            self._result = None
            for a, b, n in plan_launches(off_host, self.max_tokens_per_launch):
                if n == 0:
                    continue
                scratch = PairTable(2, self.device).reserve(2 * n)   # (its failure word goes into `pairs` with its entries)
                pairs.reserve(2 * n)
                ops.terms_accumulate(scratch.tensor, scratch.capacity, tokens, off_dev, a, b, int(off_host[a]),
                                     int(off_host[b]))
                ops.terms_fold(scratch.tensor, scratch.capacity, pairs.tensor, pairs.capacity)
                self.launches += 1
                pairs.sync()
                pairs.settle()
        return self

    def finalize(self):
        """(ids int32[K], frequency int64[K], doc_frequency int64[K]) on the device, ascending by id.  The builder stays
        usable: more ``add`` calls may follow."""
        pairs = self._pairs
        pairs.check_usable()
        if self._result is None:
            with torch.cuda.device(self.device):
                if pairs.used:
                    ids, frequency, doc_frequency = ops.terms_stats(pairs.tensor, pairs.capacity, pairs.used // 2)
                    pairs.sync()
                    ids, perm = ops.segment_sort(ids, int(ids.max()) + 1)
                    perm = perm.to(torch.int64)
                    self._result = (ids, frequency[perm], doc_frequency[perm])
                else:
                    self._result = (torch.empty(0, dtype=torch.int32, device=self.device),
                                    torch.empty(0, dtype=torch.int64, device=self.device),
                                    torch.empty(0, dtype=torch.int64, device=self.device))
        return self._result


class Dictionary:
    """The token dictionary: ``ids[index]`` is the raw id at each index, with its ``frequency`` and ``doc_frequency``
    (int64) -- ``TokenDictionary`` of the reference (token_dictionary.py:17-118) over ids instead of strings.  The tensors
    stay where they are given (host or device); the lookups run on the device, through a pair table keyed by the raw id that
    is built on first use (no dense 2^31-entry array).  ``max_doc_frequency`` is the largest ``doc_frequency`` as
    ``TokenDictionary.load`` computes it (token_dictionary.py:90), unless given."""

    def __init__(self, ids, frequency, doc_frequency, max_doc_frequency=None):
        self.ids = _as_tensor(ids, torch.int32)
        self.frequency = _as_tensor(frequency, torch.int64)
        self.doc_frequency = _as_tensor(doc_frequency, torch.int64)
        self.size = int(self.ids.numel())
        if self.frequency.numel() != self.size or self.doc_frequency.numel() != self.size:
            raise ValueError("ids, frequency and doc_frequency must have one entry per index")
        if self.size and int(self.ids.min()) < 0:
            raise ValueError("dictionary ids must be >= 0")
        if max_doc_frequency is None:
            max_doc_frequency = int(self.doc_frequency.max()) if self.size else 0
        self.max_doc_frequency = int(max_doc_frequency)
        self._lookups = {}      # device -> (table, capacity)

    @property
    def embedding_size(self):
        """token_dictionary.py:66-68: 0 is the mask, then the dictionary, then the 65536 buckets."""
        return 1 + OOV_BUCKETS + self.size

    def lookup_table(self, device, skip=None):
        """(table, capacity): raw id -> index on `device`.  `skip`: raw ids left out (the tf-idf stopwords); only the
        table without a skip set is kept."""
        device = torch.device(device)
        if skip is None and device in self._lookups:
            return self._lookups[device]
        with torch.cuda.device(device):
            keys = self.ids.to(device)
            values = torch.arange(self.size, dtype=torch.int32, device=device)
            if skip is not None and len(skip):
                keep = ~torch.isin(keys, torch.as_tensor(sorted(int(s) for s in skip), dtype=torch.int32, device=device))
                keys, values = keys[keep].contiguous(), values[keep].contiguous()
            capacity = pow2_at_least(2 * max(1, keys.numel()))
            lookup = PairTable(capacity, device, tensor=ops.terms_lookup_table(keys, values, capacity))
            used, fail = lookup.header()
            if fail or used != keys.numel():
                raise ValueError("dictionary ids must be distinct and >= 0 (%d ids, %d distinct, failure bits %d)"
                                 % (keys.numel(), used, fail))
        if skip is None:
            self._lookups[device] = (lookup.tensor, capacity)
        return lookup.tensor, capacity

    def _lookup(self, tokens, mode, oov_bucket, device):
        if isinstance(tokens, torch.Tensor) and tokens.is_cuda:
            device = tokens.device if device is None else torch.device(device)
            tokens = ops.as_ids(tokens.to(device), device).reshape(-1)
        else:
            device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
            host = check_host_tokens(tokens.numpy() if isinstance(tokens, torch.Tensor) else tokens)
            tokens = torch.from_numpy(host).to(device)
        if oov_bucket is not None:
            if isinstance(oov_bucket, torch.Tensor) and oov_bucket.is_cuda:
                if oov_bucket.numel() != tokens.numel():
                    raise ValueError("oov_bucket must hold one bucket per token: %d for %d tokens"
                                     % (oov_bucket.numel(), tokens.numel()))
                oov_bucket = ops.as_ids(oov_bucket.to(device), device).reshape(-1)
            else:
                host = check_host_buckets(oov_bucket.numpy() if isinstance(oov_bucket, torch.Tensor) else oov_bucket,
                                          tokens.numel())
                oov_bucket = torch.from_numpy(host).to(device)
        with torch.cuda.device(device):
            table, capacity = self.lookup_table(device)
            out, fail = ops.terms_lookup(tokens, table, capacity, mode, self.size, oov_bucket)
            fail = int(fail)
        if fail:
            raise ValueError("dictionary lookup refused (bits %d): %s" % (fail, failure_text(fail, FAILURES)))
        return out

    def index_of(self, tokens, device=None):
        """int32[N] on the device: the dictionary index of every token, -1 outside the dictionary
        (``get_token_index``, token_dictionary.py:104-107)."""
        return self._lookup(tokens, 0, None, device)

    def embedding_indices(self, tokens, oov_bucket=None, device=None):
        """int32[N] on the device: ``1 + index`` inside the dictionary, ``1 + size + bucket`` outside
        (``get_embedding_indices``, token_dictionary.py:58-76); bucket = ``oov_bucket[i]`` in [0, 65536) -- where a
        host-computed minhash goes -- or ``raw id & 0xFFFF`` without one."""
        return self._lookup(tokens, 1, oov_bucket, device)


def _as_tensor(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(dtype).reshape(-1).contiguous()
    return torch.from_numpy(np.array(x).reshape(-1)).to(dtype)     # (a copy: the caller's array may be read-only)


def make_token_dictionary(ids, frequency, doc_frequency, min_frequency=FLAGS.min_token_frequency,
                          max_size=FLAGS.max_token_dictionary_size):
    """make_dictionary.py:108-117: keep ``frequency >= min_frequency``, sort by frequency descending -- ties by ascending
    id, the stated deviation -- and keep the first ``min(max_size, count)``; the position is the index.  Plain torch on
    whatever device the statistics are (K entries: not the hot path)."""
    ids, frequency, doc_frequency = _as_tensor(ids, torch.int32), _as_tensor(frequency, torch.int64), \
        _as_tensor(doc_frequency, torch.int64)
    keep = frequency >= int(min_frequency)
    ids, frequency, doc_frequency = ids[keep], frequency[keep], doc_frequency[keep]
    by_id = torch.sort(ids, stable=True).indices
    order = by_id[torch.sort(frequency[by_id], descending=True, stable=True).indices]
    order = order[:max(0, min(int(max_size), int(order.numel())))]
    return Dictionary(ids[order], frequency[order], doc_frequency[order])


# ---- the TokenStat line file (proto/nlp.proto:20-31: string token = 1; uint64 frequency = 3, doc_frequency = 4, index = 5) ----
def encode_token_stat(token, frequency, doc_frequency, index):
    """One ``TokenStat`` as protobuf's proto3 serialiser writes it: fields in number order, a zero / empty one left out."""
    out = bytearray()
    text = token.encode("utf-8") if isinstance(token, str) else bytes(token)
    if text:
        out += b"\x0a" + varint(len(text)) + text
    for tag, value in ((b"\x18", frequency), (b"\x20", doc_frequency), (b"\x28", index)):
        if value:
            out += tag + varint(int(value))
    return bytes(out)


def parse_token_stat(serialized):
    """(token str, frequency, doc_frequency, index) of one ``TokenStat``, decoded from the wire format without protobuf
    (as ``cooccurrence_matrix.parse_cooccurrence_row`` does for its message); unknown fields are skipped."""
    buf = memoryview(serialized)
    n, pos = len(buf), 0
    token, values = "", {3: 0, 4: 0, 5: 0}
    while pos < n:
        key, pos = read_varint(buf, pos)
        field, wire = key >> 3, key & 7
        if wire == 0:
            val, pos = read_varint(buf, pos)
            if field in values:
                values[field] = val
        elif wire == 2:
            ln, pos = read_varint(buf, pos)
            if field == 1:
                token = bytes(buf[pos:pos + ln]).decode("utf-8")
            pos += ln
        elif wire == 5:
            pos += 4
        elif wire == 1:
            pos += 8
        else:
            raise ValueError("unsupported wire type %d in TokenStat" % wire)
    return token, values[3], values[4], values[5]


def write_dictionary(path, dictionary, token_of):
    """Writes the dictionary as the reference's line file (``TokenDictionary.save``, token_dictionary.py:26-32): one base64
    ``TokenStat`` per line, bz2, in index order -- ``TokenDictionary.load`` asserts that order.  ``token_of`` maps a raw id
    to its string (a dict, a list or a callable).  Returns the line count."""
    get = token_of if callable(token_of) else token_of.__getitem__
    ids, frequency, doc_frequency = (x.cpu().tolist() for x in (dictionary.ids, dictionary.frequency,
                                                                dictionary.doc_frequency))
    return write_lines(path, (encode_token_stat(get(raw), fr, df, index)
                              for index, (raw, fr, df) in enumerate(zip(ids, frequency, doc_frequency))))


def read_dictionary(path):
    """(tokens list of str, frequency int64[size], doc_frequency int64[size]) of a dictionary line file, in index order
    (checked, as token_dictionary.py:88 asserts it).  With the caller's interning, the dictionary is
    ``Dictionary([id_of[t] for t in tokens], frequency, doc_frequency)``."""
    tokens, frequency, doc_frequency = [], [], []
    with bz2.open(path, "rb") as f:
        for line in f:
            token, fr, df, index = parse_token_stat(base64.b64decode(line.rstrip(b"\n")))
            if index != len(tokens):
                raise ValueError("dictionary line %d carries index %d" % (len(tokens), index))
            tokens.append(token)
            frequency.append(fr)
            doc_frequency.append(df)
    return tokens, np.array(frequency, np.int64), np.array(doc_frequency, np.int64)


def main(argv=None):
    """input_file: an .npz of `tokens` / `doc_offsets` (and optionally `strings`, the token of every raw id);
    token_output: the dictionary line file."""
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--input_file", required=True, help="Input .npz of tokens / doc_offsets.")
    ap.add_argument("--token_output", required=True, help="The token dictionary output file.")
    ap.add_argument("--min_token_frequency", type=int, default=FLAGS.min_token_frequency, help="Minimum token frequency")
    ap.add_argument("--max_token_dictionary_size", type=int, default=FLAGS.max_token_dictionary_size,
                    help="Maximum size of the token dictionary.")
    args = ap.parse_args(argv)
    with np.load(args.input_file) as z:
        tokens, doc_offsets = z["tokens"], z["doc_offsets"]
        strings = z["strings"] if "strings" in z.files else None
    dictionary = make_token_dictionary(*TermStatsBuilder().add(tokens, doc_offsets).finalize(),
                                       args.min_token_frequency, args.max_token_dictionary_size)
    lines = write_dictionary(args.token_output, dictionary, (lambda i: str(strings[i])) if strings is not None else str)
    print("wrote %d tokens to %s" % (lines, args.token_output))


if __name__ == "__main__":
    main()

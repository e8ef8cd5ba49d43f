"""CPU restatements of the reference's id-level preparation stages and the inputs the term tests share.

The reference's make_dictionary.py and count_terms.py import PySpark / absl at their top and cannot be run here, so parity
rests on their source text, restated here over ids instead of strings:
  ref_stats        count_tokens + tokenstat_reducer (make_dictionary.py:67-74, 101-105): frequency = occurrences,
                   doc_frequency = documents holding the id;
  ref_dictionary   make_token_dictionary (make_dictionary.py:108-117): frequency >= min, sorted(..., reverse=True) by
                   frequency, the first min(max_size, count).  Tie rule (the build's stated deviation: the reference has
                   Spark's unspecified collect() order): ascending id;
  ref_embedding    get_embedding_index (token_dictionary.py:58-64) with the caller's bucket in place of minhash(string);
  ref_sparse_doc   make_sparse_doc (count_terms.py:44-73) in Python floats (fp64), stored as float32.  Row order (the
                   build's stated deviation): ascending index; the reference's is dict insertion order.  The norm is summed
                   in the REFERENCE's order (insertion) unless ascending=True.
counter_* are second, independent forms over collections.Counter (test_terms_host.py holds the two against each other).
"""
import functools
import math
from collections import Counter

import numpy as np

BIG = 2 ** 31 - 1
OOV_BUCKETS = 65536
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 5000]


# ---- restatement one: the reference's loops ----
def ref_stats(docs):
    """(ids, frequency, doc_frequency) int64, ascending by id."""
    frequency, doc_frequency = {}, {}
    for doc in docs:
        terms = [int(t) for t in doc]
        for term in terms:
            if term in frequency:
                frequency[term] += 1
            else:
                frequency[term] = 1
                doc_frequency[term] = 0
        for term in set(terms):
            doc_frequency[term] += 1
    ids = sorted(frequency)
    return (np.array(ids, np.int64), np.array([frequency[i] for i in ids], np.int64),
            np.array([doc_frequency[i] for i in ids], np.int64))


def ref_dictionary(ids, frequency, doc_frequency, min_frequency=20, max_size=500000):
    """(ids, frequency, doc_frequency) int64 in index order."""
    entries = sorted(zip((int(i) for i in ids), (int(f) for f in frequency), (int(d) for d in doc_frequency)))
    entries = [e for e in entries if e[1] >= min_frequency]
    entries = sorted(entries, key=lambda e: e[1], reverse=True)      # stable: ties keep ascending id
    count = max(0, min(max_size, len(entries)))
    entries = entries[:count]
    return tuple(np.array([e[k] for e in entries], np.int64) for k in range(3))


def ref_embedding(tokens, dict_ids, buckets=None):
    """(index_of int64[N] with -1 outside, embedding_index int64[N])."""
    token2index = {int(t): i for i, t in enumerate(dict_ids)}
    size = len(token2index)
    index_of, emb = [], []
    for k, t in enumerate(tokens):
        t = int(t)
        if t in token2index:
            index_of.append(token2index[t])
            emb.append(1 + token2index[t])
        else:
            index_of.append(-1)
            emb.append(1 + size + (int(buckets[k]) if buckets is not None else t & 0xFFFF))
    return np.array(index_of, np.int64), np.array(emb, np.int64)


def ref_sparse_doc(doc, token2index, doc_frequency, max_doc_frequency, stopwords, ascending=False):
    """(token_index list ascending, token_tfidf list of float32 in that order) of one document."""
    log_max_num_docs = math.log1p(max_doc_frequency)
    tf = {}
    for token in doc:
        token = int(token)
        if token in stopwords:
            continue
        if token in tf:
            tf[token] += 1.0
        else:
            tf[token] = 1.0
    row = []
    for token in tf:
        if token in token2index:
            token_index = token2index[token]
            idf = log_max_num_docs - math.log1p(int(doc_frequency[token_index])) + 1.0
            if idf < 0.0:
                idf = 0.0
            row.append((token_index, tf[token] * idf))
    norm = 0.0
    for _, tfidf in (sorted(row) if ascending else row):
        norm += tfidf * tfidf
    inorm = 1.0 / math.sqrt(norm) if norm > 0.0 else 0.0
    row.sort()
    return [r[0] for r in row], [np.float32(r[1] * inorm) for r in row]


def ref_sparse_docs(docs, dict_ids, doc_frequency, max_doc_frequency, stopwords=(), ascending=False):
    """(out_offsets int64[ndocs + 1], token_index int64[nnz], token_tfidf float32[nnz])."""
    token2index = {int(t): i for i, t in enumerate(dict_ids)}
    stopwords = set(int(s) for s in stopwords)
    offsets, index, tfidf = [0], [], []
    for doc in docs:
        i, v = ref_sparse_doc(doc, token2index, doc_frequency, max_doc_frequency, stopwords, ascending)
        index += i
        tfidf += v
        offsets.append(len(index))
    return np.array(offsets, np.int64), np.array(index, np.int64), np.array(tfidf, np.float32)


# ---- restatement two: collections.Counter ----
def counter_stats(docs):
    frequency, doc_frequency = Counter(), Counter()
    for doc in docs:
        terms = [int(t) for t in doc]
        frequency.update(terms)
        doc_frequency.update(set(terms))
    return frequency, doc_frequency


def counter_dictionary(frequency, doc_frequency, min_frequency=20, max_size=500000):
    """[(id, frequency, doc_frequency), ...] in index order: one sort on the key (-frequency, id)."""
    kept = [(-f, i) for i, f in frequency.items() if f >= min_frequency]
    return [(i, -nf, doc_frequency[i]) for nf, i in sorted(kept)[:max(0, max_size)]]


def counter_sparse_doc(doc, token2index, doc_frequency, max_doc_frequency, stopwords):
    """{index: tfidf float32} with numpy fp64 arithmetic over the whole row at once, summed ascending by index."""
    tf = Counter(int(t) for t in doc if int(t) not in stopwords and int(t) in token2index)
    if not tf:
        return {}
    index = np.array(sorted(token2index[t] for t in tf), np.int64)
    index2token = {token2index[t]: t for t in tf}
    count = np.array([tf[index2token[i]] for i in index], np.float64)
    df = np.array([doc_frequency[i] for i in index], np.float64)
    idf = np.maximum(0.0, np.log1p(np.float64(max_doc_frequency)) - np.log1p(df) + 1.0)
    tfidf = count * idf
    norm = 0.0
    for v in tfidf:
        norm += float(v) * float(v)
    inorm = 1.0 / math.sqrt(norm) if norm > 0.0 else 0.0
    return {int(i): np.float32(v * inorm) for i, v in zip(index, tfidf)}


# ---- the named cases: lists of documents over sparse provisional ids ----
def _sparse(x):
    """Dense draws -> sparse provisional ids in [0, 2^31 - 1] (an odd multiplier: distinct draws stay distinct)."""
    return ((np.asarray(x, np.int64) * 2654435761 + 12345) % (1 << 31)).astype(np.int32)


def _lengths():
    """One document per length around the wave (64) and the workgroup (256), and one of 5000; Zipf draws, so ids repeat
    inside a document and across documents."""
    rng = np.random.default_rng(11)
    return [_sparse((rng.zipf(1.3, n) - 1) % 3000) for n in LENGTHS]


def _zipf_20000():
    rng = np.random.default_rng(5)
    docs, left = [], 20000
    while left:
        n = min(left, int(rng.integers(0, 400)))
        docs.append(_sparse((rng.zipf(1.2, n) - 1) % 50000))
        left -= n
    return docs


def _cut_corpus():
    """What the cut-independence tests split: the 5000-token document between many short ones."""
    rng = np.random.default_rng(23)
    docs = [_sparse((rng.zipf(1.3, int(rng.integers(0, 60))) - 1) % 2000) for _ in range(150)]
    docs.insert(70, _sparse((rng.zipf(1.3, 5000) - 1) % 2000))
    return docs


CASES = {
    "lengths": _lengths,
    "tiny_docs_in_a_wave": lambda: [_sparse(np.random.default_rng(d).integers(0, 40, 3)) for d in range(700)],
    "one_id_5000_times": lambda: [np.full(5000, 77, np.int32)],
    "same_id_in_300_docs": lambda: [np.array([9], np.int32)] * 300,
    "extreme_ids": lambda: [np.array([0, BIG], np.int32), np.array([BIG, 5, 0, BIG - 1, BIG], np.int32),
                            np.array([BIG] * 70 + [0], np.int32), np.array([], np.int32)],
    "zipf_20000": _zipf_20000,
    "cut_corpus": _cut_corpus,
}


@functools.lru_cache(maxsize=None)
def case_docs(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_stats(name):
    """ref_stats of a case, computed once per session and shared (read-only)."""
    out = ref_stats(case_docs(name))
    for x in out:
        x.setflags(write=False)
    return out


def pack(docs):
    """An iterable of id arrays -> (tokens int32[N], doc_offsets int64[ndocs + 1])."""
    docs = [np.asarray(d, np.int32).reshape(-1) for d in docs]
    offsets = np.zeros(len(docs) + 1, np.int64)
    if docs:
        np.cumsum([len(d) for d in docs], out=offsets[1:])
    return (np.concatenate(docs) if docs else np.zeros(0, np.int32)).astype(np.int32), offsets


# ---- the tf-idf cases: (docs, dict_ids, dict_frequency, dict_doc_frequency, max_doc_frequency, stopwords) ----
CLAMPED = 424242     # the raw id whose df is above max_doc_frequency in "clamp"


def _tfidf_case(name):
    if name == "clamp":
        # idf of CLAMPED = log1p(10) - log1p(1000) + 1 < 0 -> 0: the second document has norm == 0
        docs = [np.array([5, CLAMPED, 5, 8], np.int32), np.array([CLAMPED] * 3, np.int32), np.array([8], np.int32)]
        return docs, np.array([5, CLAMPED, 8]), np.array([900, 800, 700]), np.array([3, 1000, 10]), 10, ()
    docs = list(case_docs({"lengths": "lengths", "tiny": "tiny_docs_in_a_wave", "zipf": "zipf_20000",
                           "stopwords": "zipf_20000", "one_id": "one_id_5000_times"}[name]))
    stats = ref_stats(docs)
    ids, frequency, doc_frequency = ref_dictionary(*stats, min_frequency=2 if name != "one_id" else 1, max_size=4000)
    stop = ()
    if name == "stopwords":
        stop = tuple(int(i) for i in ids[:5]) + (123456789,)          # the five most frequent ids and one that never occurs
    if name in ("zipf", "stopwords"):
        docs.insert(3, _sparse(np.arange(10 ** 6, 10 ** 6 + 30)))     # a document with no dictionary token
    return docs, ids, frequency, doc_frequency, int(doc_frequency.max()), stop


TFIDF_CASES = ["lengths", "tiny", "zipf", "stopwords", "one_id", "clamp"]


@functools.lru_cache(maxsize=None)
def tfidf_case(name):
    return _tfidf_case(name)


@functools.lru_cache(maxsize=None)
def tfidf_ref(name, ascending=False):
    docs, ids, _, df, max_df, stop = tfidf_case(name)
    out = ref_sparse_docs(docs, ids, df, max_df, stop, ascending)
    for x in out:
        x.setflags(write=False)
    return out


def ulp_distance(a, b):
    """Distance in float32 units in the last place between two arrays of non-negative finite floats."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)

"""CPU restatements of the set co-occurrence (Dice) rule of the reference's wikipedia/make_dice.py:41-54 and the inputs
the Dice tests share.

The reference's make_dice.py imports PySpark at its top and cannot be run here, so parity rests on its source text,
restated twice and independently:
  ref_dice     set, sort, double loop, dictionary of rows -- the shape of process_sdoc / increment;
  ref_counter  collections.Counter over itertools.combinations of the sorted set.
Both also count the document frequency as the builder defines it: df[id] = documents whose set contains id.
"""
import functools
from collections import Counter
from itertools import combinations

import numpy as np

MAX_DOC = 4096   # esr_dice_max_doc(); test_dice_host.py checks it against the library


def _arrays(rows, df):
    index, other, count = [], [], []
    for a in sorted(rows):
        row = rows[a]
        for b in sorted(row):
            index.append(a)
            other.append(b)
            count.append(row[b])
    ids = sorted(df)
    return (np.array(index, np.int64), np.array(other, np.int64), np.array(count, np.float32),
            np.array(ids, np.int64), np.array([df[i] for i in ids], np.float32))


def ref_dice(docs):
    """(index, other, count float32, ids, df float32), ascending by (index, other) and by id."""
    rows, df = {}, {}
    for doc in docs:
        u = sorted(set(int(x) for x in doc))
        for i in range(len(u)):
            a = u[i]
            df[a] = df.get(a, 0) + 1
            if i + 1 < len(u):
                row = rows.setdefault(a, {})
                for j in range(i + 1, len(u)):
                    b = u[j]
                    row[b] = row.get(b, 0) + 1
    return _arrays(rows, df)


def ref_counter(docs):
    """{(index, other): count}, {id: df} by Counter over combinations."""
    pairs, df = Counter(), Counter()
    for doc in docs:
        u = sorted(set(int(x) for x in doc))
        df.update(u)
        pairs.update(combinations(u, 2))
    return pairs, df


BIG = 2 ** 31 - 1
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025, MAX_DOC - 1, MAX_DOC]


def _size_docs(n):
    """One or two documents of n ids: one all distinct (every pair its own key) and one with repeats.  At the cap and one
    below it only the one with repeats (about 1160 distinct ids, 21 triangle tiles): the pure-Python restatement of a full
    triangle of 8.4 M pairs takes tens of seconds -- full_triangle_doc covers that one, with a closed-form expectation."""
    rng = np.random.default_rng(1000 + n)
    distinct = rng.choice(1 << 20, n, replace=False).astype(np.int32)
    repeats = rng.integers(0, max(2, n // 3 if n < MAX_DOC - 1 else 1200), n).astype(np.int32)
    return [repeats] if n >= MAX_DOC - 1 else [distinct, repeats]


def full_triangle_doc():
    """MAX_DOC distinct ids in random order, and what one such document gives by the rule itself -- every i < j of the
    sorted ids once, which row-major is ascending by (index, other): (doc, index, other)."""
    doc = np.random.default_rng(4096).choice(BIG, MAX_DOC, replace=False).astype(np.int32)
    u = np.sort(doc).astype(np.int64)
    i, j = np.triu_indices(MAX_DOC, 1)
    return doc, u[i], u[j]


def _cut_corpus():
    """Documents on both kernel paths: many of 0..40 ids (Zipf: frequent ids meet in most documents), some of 65..700."""
    rng = np.random.default_rng(77)
    docs = [((rng.zipf(1.3, int(rng.integers(0, 41))) - 1) % 5000).astype(np.int32) for _ in range(1500)]
    for n in (65, 100, 128, 300, 513, 700):
        docs.insert(int(rng.integers(0, len(docs))), rng.integers(0, 5000, n).astype(np.int32))
    return docs


def _row_of_1002():
    return [[0, k] for k in range(1, 1003)] + [[3, 1], [1, 2, 3]]


CASES = {"size_%d" % n: functools.partial(_size_docs, n) for n in SIZES}
CASES.update({
    "one_id_repeated": lambda: [[7] * 300, [5] * 64, [9], [3] * 65, [8, 8]],
    "primary_repeated": lambda: [[4, 9, 4, 2, 4], [1, 1, 2], [6, 5, 6] * 30],
    "extreme_ids": lambda: [[0, BIG], [BIG, 5, 0, BIG - 1], [BIG] * 3 + [0], [BIG - 1, BIG] * 40],
    "contention_3000": lambda: [[11, 5]] * 3000,
    "tiny_docs_in_a_wave": lambda: [np.random.default_rng(d).integers(0, 30, d % 5).astype(np.int32) for d in range(2000)],
    "cut_corpus": _cut_corpus,
    "row_of_1002": _row_of_1002,
})


@functools.lru_cache(maxsize=None)
def case_docs(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """ref_dice of a case, computed once per session and shared (read-only) by the tests that need it."""
    out = ref_dice(case_docs(name))
    for x in out:
        x.setflags(write=False)
    return out

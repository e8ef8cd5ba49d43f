"""CPU restatement of the co-occurrence semantics (written from the rule, not from any implementation): for each
document t[0..n) and position i, every j in range(max(0, i - W), min(n, i + W)) with t[i] > t[j] adds 1 / |i - j| to the
entry (index = t[i], other = t[j]).  W back, W - 1 forward; equal ids never pair; documents are independent.

    ref_float(docs, W)   sequential fp64 adds of 1.0 / dist in document order, then np.float32 (what the Spark job's
                         Python floats do)
    ref_exact(docs, W)   Python-integer sums of L // dist with L = lcm(1..W), then np.float32(np.float64(s) / np.float64(L))

Both return (index int64[nnz], other int64[nnz], count float32[nnz]) sorted by (index, other).
"""
import math

import numpy as np


def lcm_upto(W):
    l = 1
    for d in range(2, W + 1):
        l = l * d // math.gcd(l, d)
    return l


def _accumulate(docs, W, increment, zero):
    table = {}
    for doc in docs:
        t = [int(x) for x in doc]
        n = len(t)
        for i in range(n):
            for j in range(max(0, i - W), min(n, i + W)):
                if t[i] > t[j]:
                    key = (t[i], t[j])
                    table[key] = table.get(key, zero) + increment(abs(i - j))
    return table


def _sorted_arrays(table, to_f32):
    keys = sorted(table)
    index = np.array([k[0] for k in keys], dtype=np.int64)
    other = np.array([k[1] for k in keys], dtype=np.int64)
    count = np.array([to_f32(table[k]) for k in keys], dtype=np.float32)
    return index, other, count


def ref_float(docs, W):
    return _sorted_arrays(_accumulate(docs, W, lambda d: 1.0 / float(d), 0.0), np.float32)


def ref_exact(docs, W):
    L = lcm_upto(W)
    return _sorted_arrays(_accumulate(docs, W, lambda d: L // d, 0), lambda s: np.float32(np.float64(s) / np.float64(L)))


def ulp_distance(a, b):
    """Distance in f32 units in the last place between two arrays of positive finite floats."""
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def zipf_docs(rng, ndocs, V, max_len, a=1.3):
    """ndocs documents of 0..max_len ids in [0, V), Zipf-distributed (frequent ids repeat inside a window)."""
    docs = []
    for _ in range(ndocs):
        n = int(rng.integers(0, max_len + 1))
        docs.append(((rng.zipf(a, n) - 1) % V).astype(np.int32))
    return docs

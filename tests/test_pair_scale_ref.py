"""CPU: every vectorised oracle of tests/_pair_scale_ref.py equals its pure-Python restatement, array for array and bit for
bit -- on the small fixtures the host tests of each stage use and on one fresh random case per stage (a few thousand
tokens or entries, ties, empty documents, ids up to 2^31 - 2).  test_gpu_pair_scale.py compares the kernels only against
the vectorised oracles; this file is why it may.  It also pins the two launch thresholds those GPU cases are named for
against the text of esr_common.h.  No GPU is touched."""
import math
import os
import re

import numpy as np
import pytest

import _dice_ref as dr
import _pair_scale_ref as ps
import _terms_ref as tr
from _cooccur_ref import ref_exact, zipf_docs
from _neighbours_ref import ref_neighbours

BIG = 2 ** 31 - 2


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes()                                  # bit for bit, whatever the dtype


def _random_docs(rng, ndocs, max_len, vocabulary):
    """Documents of 0..max_len ids drawn from `vocabulary` with a Zipf law (frequent ids repeat inside a document and tie
    in frequency across the corpus), empty documents among them."""
    docs = [vocabulary[(rng.zipf(1.3, int(rng.integers(0, max_len + 1))) - 1) % vocabulary.size] for _ in range(ndocs)]
    for d in (0, ndocs // 2, ndocs // 2 + 1, ndocs - 1):
        docs[d] = vocabulary[:0]
    return docs


def _sparse_vocabulary(rng, n):
    return np.unique(np.concatenate([rng.integers(0, BIG, n), [0, 1, 255, 256, 65535, 65536, BIG - 1, BIG]])).astype(np.int64)


# ---- the thresholds ----
def test_the_thresholds_are_the_launch_rule_of_esr_common_h():
    """GRID_ELEMS and GRID_WAVES are what the cases of test_gpu_pair_scale.py must exceed to reach a grid-stride loop.  If
    the grid changes, this fails and says that those cases no longer reach what they are named for."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "esrecsys_amd", "csrc", "esr_common.h")
    with open(path) as f:
        text = f.read()
    assert re.search(r"constexpr int kWave = 64;", text)
    assert re.search(r"constexpr int kBlock = 256;", text)
    assert re.search(r"constexpr int kMaxGrid = 256 \* 8;", text)
    assert ps.GRID_BLOCKS == 256 * 8 and ps.GRID_ELEMS == 2048 * 256 == 524288 and ps.GRID_WAVES == 2048 * 4 == 8192
    table = os.path.join(os.path.dirname(path), "esr_cooccur_table.h")
    with open(table) as f:
        assert "std::min<int64_t>(kMaxGrid, cdiv(n, kBlock))" in f.read()    # grid_for: the rule the five files share


# ---- window pairs ----
@pytest.mark.parametrize("W", [1, 2, 10, 22])
@pytest.mark.parametrize("V", [3, 50, 5000])
def test_window_pairs_on_the_host_tests_corpora(W, V):
    docs = zipf_docs(np.random.default_rng(1000 * W + V), 60, V, 399)
    tokens, offsets = tr.pack(docs)
    _same(ps.vec_cooccur(tokens, offsets, W), ref_exact(docs, W))


def test_window_pairs_hand_worked():
    index, other, count = ps.vec_cooccur(*tr.pack([[5, 1, 4, 2, 3]]), 2)
    assert list(zip(index.tolist(), other.tolist(), count.tolist())) == \
        [(2, 1, 0.5), (3, 2, 1.0), (4, 1, 1.0), (4, 2, 1.0), (5, 1, 1.0)]
    _same(ps.vec_cooccur(np.zeros(0, np.int32), np.zeros(3, np.int64), 3), ref_exact([[], []], 3))


@pytest.mark.parametrize("W", [3, 7])
def test_window_pairs_fresh(W):
    rng = np.random.default_rng(100 + W)
    docs = _random_docs(rng, 90, 120, _sparse_vocabulary(rng, 300))
    docs[5] = np.array([BIG, 0] * 40)                                       # one pair, hit 79 times at distance 1
    tokens, offsets = tr.pack(docs)
    want = ref_exact(docs, W)
    assert 2000 < tokens.size and len(want[0]) > 1000 and want[0].max() == BIG
    _same(ps.vec_cooccur(tokens, offsets, W), want)


# ---- set pairs and document frequency ----
@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_set_pairs_on_the_host_tests_cases(name):
    _same(ps.vec_dice(*tr.pack(dr.case_docs(name))), dr.case_ref(name))


def test_set_pairs_fresh():
    rng = np.random.default_rng(7)
    docs = _random_docs(rng, 400, 30, _sparse_vocabulary(rng, 200))
    docs[9] = rng.choice(_sparse_vocabulary(rng, 400), 150)                 # a long one, with repeats
    docs[10] = np.array([BIG] * 5)
    tokens, offsets = tr.pack(docs)
    want = dr.ref_dice(docs)
    assert 3000 < tokens.size and want[2].max() > 3 and want[3].max() == BIG
    _same(ps.vec_dice(tokens, offsets), want)
    _same(ps.vec_dice(np.zeros(0, np.int32), np.zeros(3, np.int64)), dr.ref_dice([[], []]))


# ---- term statistics, dictionary, lookups ----
def _terms_fresh():
    rng = np.random.default_rng(31)
    vocabulary = _sparse_vocabulary(rng, 500)
    docs = _random_docs(rng, 120, 80, vocabulary)
    docs[7] = rng.choice(vocabulary, 700)                                   # a row of several hundred distinct indices
    return [np.asarray(d, np.int64) for d in docs]


@pytest.mark.parametrize("name", sorted(tr.CASES) + ["fresh"])
def test_statistics_and_dictionary(name):
    docs = _terms_fresh() if name == "fresh" else tr.case_docs(name)
    tokens, offsets = tr.pack(docs)
    want = tr.ref_stats(docs) if name == "fresh" else tr.case_stats(name)
    got = ps.vec_stats(tokens, offsets)
    _same(got, want)
    for min_frequency, max_size in ((1, 500000), (2, 7), (3, 50), (20, 500000), (1, 0)):
        _same(ps.vec_dictionary(*got, min_frequency, max_size), tr.ref_dictionary(*want, min_frequency, max_size))


def test_the_fresh_terms_case_has_ties_and_extreme_ids():
    ids, frequency, _df = tr.ref_stats(_terms_fresh())
    assert ids[0] == 0 and ids[-1] == BIG and np.bincount(frequency).max() > 20 and frequency.sum() > 3000
    cut = tr.ref_dictionary(ids, frequency, _df, 2, 50)
    assert cut[1][-1] == cut[1][-2]                                         # the cut at max_size falls inside a tie


@pytest.mark.parametrize("name", ["zipf_20000", "extreme_ids", "fresh"])
def test_lookups(name):
    docs = _terms_fresh() if name == "fresh" else tr.case_docs(name)
    tokens, _ = tr.pack(docs)
    dict_ids = tr.ref_dictionary(*tr.ref_stats(docs), 2, 300)[0]
    tokens = np.concatenate([tokens, np.array([0, tr.BIG, 65535, 65536, 12345], np.int32)])
    buckets = np.random.default_rng(3).integers(0, 65536, tokens.size).astype(np.int32)
    index, _ = tr.ref_embedding(tokens, dict_ids)
    assert (index < 0).any() and (index >= 0).any()
    _same(ps.vec_embedding(tokens, dict_ids), tr.ref_embedding(tokens, dict_ids))
    _same(ps.vec_embedding(tokens, dict_ids, buckets), tr.ref_embedding(tokens, dict_ids, buckets))
    _same(ps.vec_embedding(tokens, np.zeros(0, np.int64)), tr.ref_embedding(tokens, np.zeros(0, np.int64)))


# ---- tf-idf rows ----
@pytest.mark.parametrize("ascending", [False, True], ids=["insertion", "ascending"])
@pytest.mark.parametrize("name", tr.TFIDF_CASES)
def test_tfidf_rows_on_the_host_tests_cases(name, ascending):
    docs, ids, _, df, max_df, stop = tr.tfidf_case(name)
    tokens, offsets = tr.pack(docs)
    got = ps.vec_sparse_docs(tokens, offsets, ids, df, max_df, stop, "ascending" if ascending else "insertion")
    _same(got, tr.tfidf_ref(name, ascending))


def _python_wave_norm(squares):
    """terms_tfidf_rows_kernel's order in plain Python floats: 64 lane sums of every 64th entry, then the butterfly."""
    lanes = [0.0] * 64
    for i, x in enumerate(squares):
        lanes[i % 64] += float(x)
    for s in (1, 2, 4, 8, 16, 32):
        lanes = [lanes[l] + lanes[l ^ s] for l in range(64)]
    assert len(set(lanes)) == 1
    return lanes[0]


@pytest.mark.parametrize("name", ["lengths", "zipf", "stopwords", "clamp", "fresh"])
def test_tfidf_rows_in_the_kernels_norm_order(name):
    """The "wave" order differs from ref_sparse_docs only in the order of the norm's sum, so it is held against the
    restatement's own formula with that one sum replaced: float32(tfidf * (1 / sqrt(norm))) per row, in Python floats."""
    if name == "fresh":
        docs = _terms_fresh()
        ids, _, df = tr.ref_dictionary(*tr.ref_stats(docs), 2, 400)
        max_df, stop = int(df.max()), (int(ids[0]), 424242)
    else:
        docs, ids, _, df, max_df, stop = tr.tfidf_case(name)
    tokens, offsets = tr.pack(docs)
    off, index, tfidf = ps.vec_sparse_docs(tokens, offsets, ids, df, max_df, stop, "wave")
    a_off, a_index, a_tfidf = ps.vec_sparse_docs(tokens, offsets, ids, df, max_df, stop, "ascending")
    assert np.array_equal(off, a_off) and np.array_equal(index, a_index) and tr.ulp_distance(tfidf, a_tfidf).max() <= 1
    assert np.diff(off).max() > (64 if name != "clamp" else 2)              # rows longer than one wave are among them
    log_max = math.log1p(max_df)
    token2index = {int(t): i for i, t in enumerate(ids)}
    for d, doc in enumerate(docs):
        tf = {}
        for t in doc:
            t = int(t)
            if t not in stop and t in token2index:
                tf[token2index[t]] = tf.get(token2index[t], 0.0) + 1.0
        row = sorted(tf)
        values = [tf[i] * max(0.0, log_max - math.log1p(int(df[i])) + 1.0) for i in row]
        norm = _python_wave_norm([v * v for v in values])
        inorm = 1.0 / math.sqrt(norm) if norm > 0.0 else 0.0
        assert index[off[d]:off[d + 1]].tolist() == row
        want = np.array([np.float32(v * inorm) for v in values], np.float32)
        assert tfidf[off[d]:off[d + 1]].tobytes() == want.tobytes(), d


def test_wave_norm_is_the_lane_strided_butterfly_sum():
    rng = np.random.default_rng(2)
    lengths = np.array([0, 1, 63, 64, 65, 128, 129, 1000], np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    squares = rng.random(int(lengths.sum())) * 2.0 ** rng.integers(-30, 30, int(lengths.sum()))
    got = ps.wave_norm(squares, starts, lengths)
    want = [_python_wave_norm(squares[a:a + n]) for a, n in zip(starts, lengths)]
    assert got.tolist() == want
    sequential = [float(np.add.accumulate(squares[a:a + n])[-1]) if n else 0.0 for a, n in zip(starts, lengths)]
    assert got.tolist() != sequential                                       # (the order is visible in the bits)


# ---- neighbours ----
HAND = dict(ids=[1, 2, 3, 5, 8, 9], df=[4, 2, 2, 4, 1, 3], index=[1, 1, 1, 1, 2, 2, 3, 3, 5],
            other=[2, 3, 5, 8, 3, 5, 5, 8, 8], count=[2, 2, 4, 1, 1, 1, 2, 1, 1])     # test_neighbours_ref.py's table


@pytest.mark.parametrize("k", [1, 3, 4, 10])
@pytest.mark.parametrize("score", ["dice", "count"])
@pytest.mark.parametrize("orientation", ["stored", "both"])
def test_neighbours_hand_table(orientation, score, k):
    h = HAND
    df = h["df"] if score == "dice" else None
    _same(ps.vec_neighbours(h["index"], h["other"], h["count"], h["ids"], df, k, orientation, score),
          ref_neighbours(h["index"], h["other"], h["count"], h["ids"], df, k, orientation, score))
    _same(ps.vec_neighbours(h["other"], h["index"], h["count"], h["ids"], df, k, orientation, score),
          ref_neighbours(h["other"], h["index"], h["count"], h["ids"], df, k, orientation, score))
    if score == "count":
        _same(ps.vec_neighbours(h["index"], h["other"], h["count"], None, None, k, orientation, score),
              ref_neighbours(h["index"], h["other"], h["count"], None, None, k, orientation, score))


def _neighbours_fresh():
    """About 4000 entries over 700 sparse ids: rows of 0 to about 400 entries, small integer counts and document
    frequencies (scores tie at every k), a few counts of 0, fractional counts among them, ids without entries."""
    rng = np.random.default_rng(17)
    ids = _sparse_vocabulary(rng, 700)
    hubs = rng.choice(ids.size, 60, replace=False)
    a = ids[np.concatenate([np.full(int(n), h) for h, n in zip(hubs, rng.integers(1, 130, hubs.size))])]
    b = ids[rng.integers(0, ids.size, a.size)]
    pairs = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    count = rng.integers(0, 6, pairs.shape[0]).astype(np.float32)
    count[::7] *= np.float32(1) / np.float32(3)
    df = rng.integers(1, 5, ids.size).astype(np.float32)
    return pairs[:, 0], pairs[:, 1], count, ids, df


@pytest.mark.parametrize("k", [1, 10, 1024])
@pytest.mark.parametrize("score", ["dice", "count"])
@pytest.mark.parametrize("orientation", ["stored", "both"])
def test_neighbours_fresh(orientation, score, k):
    index, other, count, ids, df = _neighbours_fresh()
    assert index.size > 3000 and ids[-1] == BIG and np.bincount(np.searchsorted(ids, np.concatenate([index, other]))).max() > 64
    want = ref_neighbours(index, other, count, ids, df, k, orientation, score)
    _same(ps.vec_neighbours(index, other, count, ids, df, k, orientation, score), want)
    if k == 10:
        full = want[4] == k
        assert full.any() and (want[2][full, 1:] == want[2][full, :-1]).any()        # ties inside the kept rows


def test_neighbours_edges():
    e = np.zeros(0, np.int64)
    _same(ps.vec_neighbours(e, e, e, [4, 7, BIG], [1.0, 1.0, 2.0], 10), ref_neighbours(e, e, e, [4, 7, BIG], [1.0, 1.0, 2.0], 10))
    _same(ps.vec_neighbours(e, e, e, None, None, 10, "both", "count"), ref_neighbours(e, e, e, None, None, 10, "both", "count"))
    with pytest.raises(KeyError):
        ps.vec_neighbours([1, 4], [2, 5], [1, 1], [1, 2, 5], [1, 1, 1], 2)

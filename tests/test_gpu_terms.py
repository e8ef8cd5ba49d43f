"""GPU: term statistics, the dictionary lookup and tf-idf documents (esr_terms.hip, wikipedia/make_dictionary.py,
wikipedia/count_terms.py) against the CPU restatements of tests/_terms_ref.py.

Counts, ids, indices and offsets are compared BIT FOR BIT: the sums are integers, so nothing depends on atomic order or on
how the corpus is cut.  token_tfidf is held within 1 float32 ulp of float32(restatement) -- a derived bound: the device
differs from the restatement only in the order of an fp64 sum of n squares (ascending index, lane-strided, against
insertion order), a relative error of at most about n 2^-53, which can move the float32 rounding only at a tie -- and at
least 99 % of the entries must compare bit-equal (test_terms_host.py checks on the CPU that the restatement itself keeps
that when summed in ascending order).

The reference's make_dictionary.py / count_terms.py import PySpark / absl at their top and cannot be run here: parity rests
on their source text, restated twice in tests/_terms_ref.py."""
import numpy as np
import pytest
import torch

import _terms_ref as tr

from esrecsys_amd.wikipedia import count_terms as ct
from esrecsys_amd.wikipedia import make_cooccurrence as mc
from esrecsys_amd.wikipedia import make_dictionary as mk

pytestmark = pytest.mark.gpu


def _check_stats(builder, expect):
    ids, frequency, doc_frequency = builder.finalize()
    assert ids.is_cuda and ids.dtype == torch.int32 and frequency.dtype == torch.int64 and doc_frequency.dtype == torch.int64
    assert ids.cpu().to(torch.int64).tolist() == expect[0].tolist()
    assert np.array_equal(frequency.cpu().numpy(), expect[1])
    assert np.array_equal(doc_frequency.cpu().numpy(), expect[2])
    assert builder.num_ids == len(expect[0])


# ---- statistics ----
@pytest.mark.parametrize("name", ["lengths", "tiny_docs_in_a_wave", "one_id_5000_times", "same_id_in_300_docs",
                                  "extreme_ids", "zipf_20000"])
def test_statistics_equal_the_restatement(dev, name):
    """Document lengths 0, 1, 63, 64, 65, 255, 256, 257 and 5000; document boundaries inside a wave (700 documents of 3
    tokens); one document of 5000 copies of one id; 300 documents holding the same id once; ids 0 and 2^31 - 1; a
    20 000-token Zipf corpus."""
    b = mk.TermStatsBuilder(capacity=64, device=dev).add(*tr.pack(tr.case_docs(name)))
    _check_stats(b, tr.case_stats(name))


def test_hot_id_counts(dev):
    b = mk.TermStatsBuilder(capacity=8, device=dev).add(*tr.pack(tr.case_docs("one_id_5000_times")))
    assert [x.tolist() for x in b.finalize()] == [[77], [5000], [1]]
    b = mk.TermStatsBuilder(capacity=8, device=dev).add(*tr.pack(tr.case_docs("same_id_in_300_docs")))
    assert [x.tolist() for x in b.finalize()] == [[9], [300], [300]]
    ids = mk.TermStatsBuilder(device=dev).add(*tr.pack(tr.case_docs("extreme_ids"))).finalize()[0]
    assert ids.tolist() == [0, 5, tr.BIG - 1, tr.BIG]


def test_no_documents(dev):
    b = mk.TermStatsBuilder(capacity=8, device=dev)
    b.add(np.zeros(0, np.int32), np.zeros(1, np.int64)).add(np.zeros(0, np.int32), np.zeros(4, np.int64))
    ids, frequency, doc_frequency = b.finalize()
    assert ids.numel() == frequency.numel() == doc_frequency.numel() == 0 and ids.is_cuda and b.launches == 0


# ---- cut independence ----
def test_one_add_per_document(dev):
    docs = tr.case_docs("cut_corpus")
    b = mk.TermStatsBuilder(capacity=1 << 14, device=dev)
    for d in docs:
        b.add(*tr.pack([d]))
    _check_stats(b, tr.case_stats("cut_corpus"))
    assert b.launches == sum(1 for d in docs if len(d))
    b.finalize()
    b.add(*tr.pack(docs))                                        # the builder stays usable after finalize
    ids, frequency, doc_frequency = b.finalize()
    expect = tr.case_stats("cut_corpus")
    assert np.array_equal(frequency.cpu().numpy(), 2 * expect[1]) and np.array_equal(doc_frequency.cpu().numpy(), 2 * expect[2])


@pytest.mark.parametrize("kw", [dict(), dict(max_tokens_per_launch=100), dict(capacity=8),
                                dict(capacity=8, max_tokens_per_launch=1000)], ids=str)
def test_cuts_and_growth_do_not_change_the_result(dev, kw):
    """One add; a launch budget of 100 tokens, which the 5000-token document exceeds (its own launch, uncut); a table of 8
    slots, rehashed many times (a table is made at its first launch's size, so growth needs a second launch: with the
    default budget the corpus comes in three adds, with a budget of 1000 tokens in one)."""
    docs = tr.case_docs("cut_corpus")
    tokens, off = tr.pack(docs)
    limit = kw.get("max_tokens_per_launch", 1 << 21)
    b = mk.TermStatsBuilder(device=dev, **kw)
    if kw == dict(capacity=8):
        for part in (docs[:5], docs[5:60], docs[60:]):
            b.add(*tr.pack(part))
        assert b.launches == 3
    else:
        b.add(torch.from_numpy(tokens).to(dev), torch.from_numpy(off).to(dev))
        assert b.launches == len([p for p in mk.plan_launches(off, limit) if p[2]])
    _check_stats(b, tr.case_stats("cut_corpus"))
    if kw.get("capacity") == 8:
        assert b.rehashes > (1 if limit == 1000 else 0)
    if limit == 100:
        assert b.launches > 50
    assert b.capacity >= 2 * (2 * b.num_ids)                         # two slots per id, load factor at most 1/2


# ---- failures ----
def test_negative_id_on_the_device_leaves_the_builder_unusable(dev):
    b = mk.TermStatsBuilder(capacity=64, device=dev)
    b.add(np.array([1, 2, 3], np.int32), np.array([0, 3], np.int64))
    with pytest.raises(mc.CooccurrenceError, match="negative id"):
        b.add(torch.tensor([4, -5, 6], dtype=torch.int32, device=dev), np.array([0, 2, 3], np.int64))
    with pytest.raises(mc.CooccurrenceError, match="unusable"):
        b.add(np.array([1], np.int32), np.array([0, 1], np.int64))
    with pytest.raises(mc.CooccurrenceError, match="unusable"):
        b.finalize()


def test_bad_input_is_refused_on_the_host_before_any_launch(dev):
    b = mk.TermStatsBuilder(capacity=64, device=dev)
    tokens = np.array([1, 2, 3], np.int32)
    for off in ([1, 3], [0, 2], [0, 2, 1, 3], []):
        with pytest.raises(ValueError, match="doc_offsets"):
            b.add(tokens, np.array(off, np.int64))
        with pytest.raises(ValueError, match="doc_offsets"):
            b.add(torch.from_numpy(tokens).to(dev), torch.tensor(off, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="token ids"):
        b.add(np.array([1, -2, 3], np.int32), np.array([0, 3], np.int64))
    assert b.launches == 0 and b.rehashes == 0 and b.capacity == 64 and b._pairs.tensor is None
    b.add(tokens, np.array([0, 3], np.int64))                     # a refusal on the host leaves the builder usable
    assert b.finalize()[0].tolist() == [1, 2, 3]


# ---- dictionary ----
@pytest.fixture(scope="module")
def zipf_dictionary(dev):
    tokens, off = tr.pack(tr.case_docs("zipf_20000"))
    stats = mk.TermStatsBuilder(capacity=1 << 12, device=dev).add(tokens, off).finalize()
    return mk.make_token_dictionary(*stats, min_frequency=2, max_size=300)


def test_dictionary_equals_the_restatement(dev, zipf_dictionary):
    d = zipf_dictionary
    ids, frequency, df = tr.ref_dictionary(*tr.case_stats("zipf_20000"), min_frequency=2, max_size=300)
    assert d.ids.is_cuda and d.size == 300 == len(ids) and d.embedding_size == 1 + 65536 + 300
    assert d.ids.cpu().to(torch.int64).tolist() == ids.tolist() and d.frequency.tolist() == frequency.tolist()
    assert d.doc_frequency.tolist() == df.tolist() and d.max_doc_frequency == int(df.max())


def test_lookups_equal_the_restatement(dev, zipf_dictionary):
    d = zipf_dictionary
    tokens = np.concatenate([tr.pack(tr.case_docs("zipf_20000"))[0], np.array([0, tr.BIG, 65535, 65536], np.int32)])
    buckets = np.random.default_rng(3).integers(0, 65536, tokens.size).astype(np.int32)
    buckets[:4] = [0, 65535, 1, 65534]
    ids = d.ids.cpu().numpy()
    e_index, e_default = tr.ref_embedding(tokens, ids)
    _, e_bucket = tr.ref_embedding(tokens, ids, buckets)
    outside = e_index < 0
    assert 0.02 < outside.mean() < 0.9                              # both sides of the dictionary are exercised
    got = d.index_of(tokens, device=dev)
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), e_index)
    dev_tokens = torch.from_numpy(tokens).to(dev)
    assert np.array_equal(d.embedding_indices(dev_tokens).cpu().numpy(), e_default)
    got = d.embedding_indices(dev_tokens, torch.from_numpy(buckets).to(dev)).cpu().numpy()
    assert np.array_equal(got, e_bucket) and np.array_equal(d.embedding_indices(tokens, buckets, device=dev).cpu().numpy(), e_bucket)
    assert np.array_equal(got[outside], 1 + d.size + buckets[outside].astype(np.int64))
    assert np.array_equal(e_default[outside], 1 + d.size + (tokens[outside].astype(np.int64) & 0xFFFF))
    assert got.max() < d.embedding_size and got.min() >= 1
    assert d.index_of(np.zeros(0, np.int32), device=dev).numel() == 0


def test_lookup_of_extreme_ids_and_an_empty_dictionary(dev):
    d = mk.Dictionary([tr.BIG, 0, 7], [3, 2, 1], [1, 1, 1])
    assert d.index_of([0, 7, tr.BIG, 1, tr.BIG - 1], device=dev).tolist() == [1, 2, 0, -1, -1]
    assert d.embedding_indices([7, 65536 + 9], device=dev).tolist() == [3, 1 + 3 + 9]
    empty = mk.Dictionary([], [], [])
    assert empty.index_of([4, 5], device=dev).tolist() == [-1, -1]
    assert empty.embedding_indices([4, 5], [100, 65535], device=dev).tolist() == [101, 65536]


def test_lookup_refuses_bad_arguments(dev, zipf_dictionary):
    d = zipf_dictionary
    with pytest.raises(ValueError, match="token ids"):
        d.index_of([1, -1], device=dev)
    with pytest.raises(ValueError, match="negative id"):
        d.index_of(torch.tensor([1, -1], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="oov_bucket"):
        d.embedding_indices([1, 2], [0, 65536], device=dev)
    with pytest.raises(ValueError, match="oov_bucket"):
        d.embedding_indices(torch.tensor([1, 2], dtype=torch.int32, device=dev),
                            torch.tensor([0, 65536], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="oov_bucket"):
        d.embedding_indices([1, 2], [0], device=dev)
    with pytest.raises(ValueError, match="distinct"):
        mk.Dictionary([5, 5], [1, 1], [1, 1]).index_of([5], device=dev)
    assert d.index_of([int(d.ids[0])], device=dev).tolist() == [0]      # the dictionary stays usable


def test_the_chain_is_closed(dev, zipf_dictionary):
    """Raw ids -> embedding indices on the device -> CooccurrenceBuilder equals process_docs on the restatement's indices."""
    docs = tr.case_docs("zipf_20000")[:40]
    tokens, off = tr.pack(docs)
    emb = zipf_dictionary.embedding_indices(torch.from_numpy(tokens).to(dev))
    got = mc.CooccurrenceBuilder(5, capacity=1 << 10, device=dev).add(emb, off).finalize()
    e_emb = tr.ref_embedding(tokens, zipf_dictionary.ids.cpu().numpy())[1]
    expect = mc.process_docs([e_emb[off[d]:off[d + 1]] for d in range(len(docs))], 5, device=dev)
    assert got[0].numel() > 1000
    for g, e in zip(got, expect):
        assert torch.equal(g, e)


# ---- tf-idf ----
def _tfidf_builder(dev, name, **kw):
    docs, ids, frequency, df, max_df, stop = tr.tfidf_case(name)
    d = mk.Dictionary(ids, frequency, df, max_doc_frequency=max_df)
    return ct.TfidfBuilder(d, stopwords=set(stop), device=dev, **kw), tr.pack(docs)


def _check_tfidf(result, name):
    e_off, e_index, e_tfidf = tr.tfidf_ref(name)
    off, index, tfidf = result
    assert off.is_cuda and off.dtype == torch.int64 and index.dtype == torch.int32 and tfidf.dtype == torch.float32
    assert np.array_equal(off.cpu().numpy(), e_off)
    assert np.array_equal(index.cpu().numpy().astype(np.int64), e_index)
    got = tfidf.cpu().numpy()
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    ulps = tr.ulp_distance(got, e_tfidf)
    print("%s: nnz %d, max ulp %d, bit-equal %.5f" % (name, ulps.size, ulps.max(), (ulps == 0).mean()))
    assert ulps.max() <= 1
    assert (ulps == 0).mean() >= 0.99
    # every non-empty row with positive norm is a unit vector up to the float32 rounding of its n entries
    sq = np.concatenate([[0.0], np.cumsum(got.astype(np.float64) ** 2)])
    n = np.diff(e_off)
    norm = sq[e_off[1:]] - sq[e_off[:-1]]
    zero = np.array([not np.any(got[a:b]) for a, b in zip(e_off[:-1], e_off[1:])])
    rows = (n > 0) & ~zero
    assert np.all(np.abs(norm[rows] - 1.0) <= n[rows] * 2.0 ** -23)
    return got


@pytest.mark.parametrize("name", tr.TFIDF_CASES)
def test_tfidf_equals_the_restatement(dev, name):
    """The length and boundary cases of the statistics; a stopword set; a document with no dictionary token; a df above
    max_doc_frequency (the clamp at 0 fires, and a document made only of that token has norm == 0)."""
    builder, (tokens, off) = _tfidf_builder(dev, name)
    got = _check_tfidf(builder.transform(tokens, off), name)
    again = builder.transform(torch.from_numpy(tokens).to(dev), torch.from_numpy(off).to(dev))[2].cpu().numpy()
    assert np.array_equal(got.view(np.int32), again.view(np.int32))      # a repeated transform: identical bits


def test_tfidf_clamp_and_zero_norm(dev):
    builder, (tokens, off) = _tfidf_builder(dev, "clamp")
    out_off, index, tfidf = builder.transform(tokens, off)
    assert out_off.tolist() == [0, 3, 4, 5] and index.tolist() == [0, 1, 2, 1, 2]
    assert tfidf[1] == 0 and tfidf[3] == 0 and tfidf[4] == 1 and tfidf[0] > 0


@pytest.mark.parametrize("name,limit", [("lengths", 100), ("zipf", 1000), ("tiny", 64)])
def test_tfidf_does_not_depend_on_the_launch_budget(dev, name, limit):
    builder, (tokens, off) = _tfidf_builder(dev, name, max_tokens_per_launch=limit)
    _check_tfidf(builder.transform(tokens, off), name)
    assert builder.launches > 3


def test_tfidf_empty_inputs(dev):
    builder, _ = _tfidf_builder(dev, "clamp")
    off, index, tfidf = builder.transform(np.zeros(0, np.int32), np.zeros(4, np.int64))
    assert off.tolist() == [0, 0, 0, 0] and index.numel() == tfidf.numel() == 0 and index.is_cuda
    off, index, tfidf = builder.transform(np.zeros(0, np.int32), np.zeros(1, np.int64))
    assert off.tolist() == [0] and index.numel() == 0
    empty = ct.TfidfBuilder(mk.Dictionary([], [], []), device=dev)
    assert empty.transform(np.array([1, 2], np.int32), np.array([0, 1, 2], np.int64))[0].tolist() == [0, 0, 0]


def test_tfidf_failures(dev):
    builder, _ = _tfidf_builder(dev, "clamp")
    with pytest.raises(ValueError, match="doc_offsets"):
        builder.transform(np.array([5, 8], np.int32), np.array([0, 1], np.int64))
    assert builder.launches == 0
    with pytest.raises(mc.CooccurrenceError, match="negative id"):
        builder.transform(torch.tensor([5, -8], dtype=torch.int32, device=dev), np.array([0, 2], np.int64))
    with pytest.raises(mc.CooccurrenceError, match="unusable"):
        builder.transform(np.array([5, 8], np.int32), np.array([0, 2], np.int64))

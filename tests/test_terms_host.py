"""CPU: the host side of the term stages (wikipedia/make_dictionary.py, wikipedia/count_terms.py) -- the two restatements
of tests/_terms_ref.py against each other on every named case, launch planning, ranking, the line files' bytes and the
argument checks.  No GPU is touched."""
import base64
import bz2
import struct

import numpy as np
import pytest
import torch

import _terms_ref as tr

from esrecsys_amd.wikipedia import count_terms as ct
from esrecsys_amd.wikipedia import make_dictionary as mk


# ---- the restatement against the Counter form ----
@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_stats_restatements_agree(name):
    ids, frequency, doc_frequency = tr.case_stats(name)
    cf, cdf = tr.counter_stats(tr.case_docs(name))
    assert ids.tolist() == sorted(cf)
    assert frequency.tolist() == [cf[i] for i in ids.tolist()]
    assert doc_frequency.tolist() == [cdf[i] for i in ids.tolist()]
    assert int(frequency.sum()) == sum(len(d) for d in tr.case_docs(name))


@pytest.mark.parametrize("name", sorted(tr.CASES))
@pytest.mark.parametrize("min_frequency,max_size", [(1, 500000), (2, 7), (20, 500000)])
def test_dictionary_restatements_agree(name, min_frequency, max_size):
    ids, frequency, doc_frequency = tr.ref_dictionary(*tr.case_stats(name), min_frequency, max_size)
    expect = tr.counter_dictionary(*tr.counter_stats(tr.case_docs(name)), min_frequency, max_size)
    assert list(zip(ids.tolist(), frequency.tolist(), doc_frequency.tolist())) == expect


@pytest.mark.parametrize("name", tr.TFIDF_CASES)
def test_sparse_doc_restatements_agree(name):
    """The loop form (norm summed in the reference's insertion order) against the numpy / Counter form (ascending): the
    same indices, values within 1 float32 ulp."""
    docs, ids, _, df, max_df, stop = tr.tfidf_case(name)
    off, index, tfidf = tr.tfidf_ref(name)
    token2index = {int(t): i for i, t in enumerate(ids)}
    assert off.size == len(docs) + 1
    for d, doc in enumerate(docs):
        row = tr.counter_sparse_doc(doc, token2index, df, max_df, set(stop))
        a, b = off[d], off[d + 1]
        assert index[a:b].tolist() == sorted(row)
        assert np.all(tr.ulp_distance(tfidf[a:b], np.array([row[i] for i in sorted(row)], np.float32)) <= 1)


@pytest.mark.parametrize("name", tr.TFIDF_CASES)
def test_ascending_norm_order_keeps_99_percent_of_the_bits(name):
    """What test_gpu_terms.py relies on: summing the norm in ascending-index order (the device's order of terms, up to its
    tree) instead of insertion order moves the float32 result by at most 1 ulp, and leaves at least 99 % bit-equal."""
    _, index, tfidf = tr.tfidf_ref(name)
    off2, index2, tfidf2 = tr.tfidf_ref(name, True)
    assert np.array_equal(index, index2) and np.array_equal(tr.tfidf_ref(name)[0], off2)
    d = tr.ulp_distance(tfidf, tfidf2)
    assert d.size and d.max() <= 1 and (d == 0).mean() >= 0.99


def test_tfidf_cases_hold_what_they_are_for():
    off, index, tfidf = tr.tfidf_ref("clamp")
    assert off.tolist() == [0, 3, 4, 5] and index.tolist() == [0, 1, 2, 1, 2]
    assert tfidf[1] == 0 and tfidf[3] == 0 and tfidf[4] == 1            # the clamp fired; the norm == 0 row is all 0
    off, _, _ = tr.tfidf_ref("zipf")
    assert off[3] == off[4]                                              # the document with no dictionary token
    assert tr.tfidf_ref("stopwords")[1].size < tr.tfidf_ref("zipf")[1].size
    assert np.diff(tr.tfidf_ref("lengths")[0])[0] == 0                   # the empty document
    assert tr.tfidf_ref("one_id")[2].tolist() == [1.0]


def test_idf_table_is_the_formula_as_written():
    df = np.array([1, 3, 10, 1000, 0])
    idf = ct.idf_table(df, 10)
    assert idf.dtype == np.float64
    assert idf.tolist() == [max(0.0, float(np.log1p(10) - np.log1p(x) + 1.0)) for x in df.tolist()]
    assert idf[3] == 0.0 and idf[2] == 1.0
    assert np.array_equal(ct.idf_table(torch.from_numpy(df), 10), idf)


# ---- launch planning ----
def _check_plan(off, limit):
    plan = mk.plan_launches(off, limit)
    assert [p[0] for p in plan] == [0] + [p[1] for p in plan[:-1]] and (not plan or plan[-1][1] == off.size - 1)
    for a, b, n in plan:
        assert b > a and n == off[b] - off[a]
        assert n <= limit or b == a + 1                                 # above the budget only ALONE
    return plan


def test_plan_covers_whole_documents_only():
    off = tr.pack(tr.case_docs("cut_corpus"))[1]
    for limit in (1, 100, 257, 5000, 1 << 30):
        plan = _check_plan(off, limit)
        if limit == 100:
            assert (70, 71, 5000) in plan                               # the long document alone, uncut
        if limit == 1 << 30:
            assert plan == [(0, off.size - 1, int(off[-1]))]


def test_plan_with_empty_documents_and_none():
    assert mk.plan_launches(np.zeros(1, np.int64), 10) == []
    assert _check_plan(np.zeros(5, np.int64), 10) == [(0, 4, 0)]
    assert _check_plan(np.array([0, 0, 3, 3, 3, 9, 9], np.int64), 4) == [(0, 4, 3), (4, 5, 6), (5, 6, 0)]
    assert _check_plan(np.array([0, 4, 8], np.int64), 4) == [(0, 1, 4), (1, 2, 4)]


# ---- the shared planner (wikipedia/pair_table.py), on the inputs of the two plan_launches tests ----
def _dice_plan_offsets(limit):
    """test_dice_host.py's input for `limit`: lengths 0..11, empty documents, 300, 1, the cap, 0..69."""
    from _dice_ref import MAX_DOC
    rng = np.random.default_rng(limit)
    lens = np.concatenate([rng.integers(0, 12, 400), [0, 0, 300, 1, MAX_DOC, 0], rng.integers(0, 70, 100), [0]])
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


# What both public plan_launches returned before plan_ranges existed: (ranges, crc32 of the int64 [ranges, 3] array) for
# every limit of the two existing tests, and the lists themselves where they are short.
DICE_PLANS = {1: (498, 1447092877), 7: (472, 967786916), 100: (234, 567998729), 5000: (23, 517427679),
              1 << 26: (1, 128799818)}
DICE_PLAN_5000 = [(0, 202, 4956), (202, 402, 4901), (402, 403, 45150), (403, 404, 1), (404, 405, 8390656), (405, 411, 4969),
                  (411, 419, 4831), (419, 424, 2957), (424, 432, 4931), (432, 439, 4531), (439, 446, 4979), (446, 451, 4127),
                  (451, 453, 3975), (453, 458, 4374), (458, 466, 4479), (466, 470, 4603), (470, 475, 4823), (475, 479, 4642),
                  (479, 484, 4833), (484, 494, 4960), (494, 498, 4674), (498, 502, 4857), (502, 507, 2524)]
TERMS_PLANS = {1: (150, 2274331956), 100: (54, 1619156526), 257: (20, 2812722372), 5000: (3, 1310867510),
               1 << 30: (1, 1960462011)}
TERMS_PLAN_257 = [(0, 7, 209), (7, 13, 240), (13, 22, 253), (22, 30, 225), (30, 38, 227), (38, 46, 256), (46, 54, 235),
                  (54, 62, 254), (62, 69, 237), (69, 70, 53), (70, 71, 5000), (71, 81, 229), (81, 90, 241), (90, 98, 226),
                  (98, 106, 245), (106, 117, 240), (117, 123, 253), (123, 135, 254), (135, 144, 257), (144, 151, 230)]
TERMS_PLAN_5000 = [(0, 70, 2189), (70, 71, 5000), (71, 151, 2175)]


def _check_ranges(cum, limit):
    from esrecsys_amd.wikipedia.pair_table import plan_ranges
    plan = plan_ranges(cum, limit)
    n = len(cum) - 1
    covered = np.zeros(n, np.int64)
    for (a, b, cost), nxt in zip(plan, plan[1:] + [None]):
        assert 0 <= a < b <= n and cost == cum[b] - cum[a]
        assert cost <= limit or b == a + 1                              # above the limit only as ONE document
        assert nxt is None or nxt[0] == b                               # consecutive
        covered[a:b] += 1
    assert np.all(covered == 1) and (not n or (plan[0][0] == 0 and plan[-1][1] == n))     # [0, ndocs) exactly once
    return plan


def _digest(plan):
    import zlib
    return len(plan), zlib.crc32(np.array(plan, np.int64).tobytes())


def test_plan_ranges_is_what_both_plan_launches_were():
    from esrecsys_amd.wikipedia import make_dice as md
    from esrecsys_amd.wikipedia.pair_table import plan_ranges
    for limit, want in DICE_PLANS.items():
        off = _dice_plan_offsets(limit)
        cum = np.concatenate([[0], np.cumsum(md.pair_bounds(off))])
        plan = _check_ranges(cum, limit)
        assert md.plan_launches(off, limit) == plan and _digest(plan) == want
    assert md.plan_launches(_dice_plan_offsets(5000), 5000) == DICE_PLAN_5000
    off = tr.pack(tr.case_docs("cut_corpus"))[1]
    for limit, want in TERMS_PLANS.items():
        plan = _check_ranges(off, limit)
        assert mk.plan_launches(off, limit) == plan and _digest(plan) == want
    assert mk.plan_launches(off, 257) == TERMS_PLAN_257 and mk.plan_launches(off, 5000) == TERMS_PLAN_5000
    for limit in (0, 1, 10):                                            # no documents: no range
        assert plan_ranges(np.zeros(1, np.int64), limit) == []
    assert _digest(DICE_PLAN_5000) == DICE_PLANS[5000] and _digest(TERMS_PLAN_257) == TERMS_PLANS[257]


# ---- ranking ----
def test_ranking_ties_go_by_ascending_id():
    ids = np.array([50, 7, 9, 3, 100, 8])
    frequency = np.array([5, 9, 5, 5, 1, 9])
    df = np.array([1, 2, 3, 4, 1, 6])
    d = mk.make_token_dictionary(ids, frequency, df, min_frequency=2, max_size=100)
    assert d.ids.tolist() == [7, 8, 3, 9, 50] and d.frequency.tolist() == [9, 9, 5, 5, 5]
    assert d.doc_frequency.tolist() == [2, 6, 4, 3, 1] and d.size == 5 and d.max_doc_frequency == 6
    assert d.embedding_size == 1 + 65536 + 5
    assert d.ids.dtype == torch.int32 and d.frequency.dtype == torch.int64 and d.doc_frequency.dtype == torch.int64


@pytest.mark.parametrize("max_size,expect", [(0, []), (1, [7]), (3, [7, 8, 3]), (6, [7, 8, 3, 9, 50, 100]),
                                             (1000, [7, 8, 3, 9, 50, 100])])
def test_max_size_edges(max_size, expect):
    d = mk.make_token_dictionary([50, 7, 9, 3, 100, 8], [5, 9, 5, 5, 1, 9], [1] * 6, min_frequency=0, max_size=max_size)
    assert d.ids.tolist() == expect and d.size == len(expect)
    assert d.max_doc_frequency == (1 if expect else 0)


@pytest.mark.parametrize("min_frequency,expect", [(0, 6), (1, 6), (2, 5), (5, 5), (6, 2), (9, 2), (10, 0)])
def test_min_frequency_edges(min_frequency, expect):
    d = mk.make_token_dictionary([50, 7, 9, 3, 100, 8], [5, 9, 5, 5, 1, 9], [1] * 6, min_frequency, 100)
    assert d.size == expect


def test_defaults_are_the_reference_flags():
    assert mk.FLAGS.min_token_frequency == 20 and mk.FLAGS.max_token_dictionary_size == 500000
    d = mk.make_token_dictionary([1, 2], [19, 20], [1, 1])
    assert d.ids.tolist() == [2]


@pytest.mark.parametrize("name", ["zipf_20000", "extreme_ids"])
def test_ranking_equals_the_restatement(name):
    stats = tr.case_stats(name)
    for min_frequency, max_size in ((1, 500000), (3, 50)):
        d = mk.make_token_dictionary(*stats, min_frequency, max_size)
        ids, frequency, df = tr.ref_dictionary(*stats, min_frequency, max_size)
        assert d.ids.tolist() == ids.tolist() and d.frequency.tolist() == frequency.tolist()
        assert d.doc_frequency.tolist() == df.tolist()


# ---- the line files ----
def _v(x):
    out = b""
    while x > 0x7F:
        out += bytes([(x & 0x7F) | 0x80])
        x >>= 7
    return out + bytes([x])


def test_dictionary_file_bytes_and_round_trip(tmp_path):
    d = mk.Dictionary([40, 7, 300], [1000, 300, 5], [130, 0, 2])
    names = {40: "the", 7: "café", 300: ""}
    path = str(tmp_path / "tokens.pb.b64.bz2")
    assert mk.write_dictionary(path, d, names) == 3
    with bz2.open(path, "rb") as f:
        lines = f.read().split(b"\n")
    assert lines[-1] == b"" and len(lines) == 4
    # TokenStat: token = 1 (string), frequency = 3, doc_frequency = 4, index = 5; zero / empty fields are left out
    hand = [b"\x0a\x03the" + b"\x18" + _v(1000) + b"\x20" + _v(130),
            b"\x0a\x05caf\xc3\xa9" + b"\x18" + _v(300) + b"\x28\x01",
            b"\x18\x05" + b"\x20\x02" + b"\x28\x02"]
    assert [base64.b64decode(x) for x in lines[:3]] == hand
    assert _v(1000) == b"\xe8\x07" and _v(130) == b"\x82\x01"
    tokens, frequency, df = mk.read_dictionary(path)
    assert tokens == ["the", "café", ""] and frequency.tolist() == [1000, 300, 5] and df.tolist() == [130, 0, 2]
    assert frequency.dtype == np.int64 and df.dtype == np.int64
    assert mk.write_dictionary(path, d, lambda i: names[i]) == 3 and mk.read_dictionary(path)[0] == tokens


def test_read_dictionary_checks_the_index_order(tmp_path):
    path = str(tmp_path / "bad.bz2")
    with bz2.open(path, "wb") as f:
        f.write(base64.b64encode(mk.encode_token_stat("a", 1, 1, 0)) + b"\n")
        f.write(base64.b64encode(mk.encode_token_stat("b", 1, 1, 2)) + b"\n")
    with pytest.raises(ValueError, match="index 2"):
        mk.read_dictionary(path)


def test_sparse_docs_file_bytes(tmp_path):
    path = str(tmp_path / "sparse.pb.b64.bz2")
    off = np.array([0, 2, 2, 3], np.int64)
    index = np.array([3, 300, 0], np.int32)
    tfidf = np.array([0.6, 0.8, 1.0], np.float32)
    assert ct.write_sparse_docs(path, [17, 0, 200], torch.from_numpy(off), index, tfidf) == 3
    with bz2.open(path, "rb") as f:
        lines = f.read().split(b"\n")
    # SparseDocument: primary_index = 2 (varint), token_index = 4 (packed varints), token_tfidf = 5 (packed floats)
    hand = [b"\x10\x11" + b"\x22\x03\x03\xac\x02" + b"\x2a\x08" + struct.pack("<2f", 0.6, 0.8),
            b"",
            b"\x10\xc8\x01" + b"\x22\x01\x00" + b"\x2a\x04" + struct.pack("<f", 1.0)]
    assert [base64.b64decode(x) for x in lines[:3]] == hand and lines[3:] == [b""]
    assert ct.write_sparse_docs(path, None, off, index, tfidf) == 3
    with pytest.raises(ValueError, match="one index per document"):
        ct.write_sparse_docs(path, [1, 2], off, index, tfidf)


# ---- argument errors, refused on the host ----
def test_negative_or_oversized_id_is_refused():
    with pytest.raises(ValueError, match="token ids"):
        mk.check_host_tokens([3, -1, 4])
    with pytest.raises(ValueError, match="token ids"):
        mk.check_host_tokens(np.array([3, 2 ** 31], np.int64))
    assert mk.check_host_tokens(np.array([[0, 2 ** 31 - 1]], np.int64)).tolist() == [0, 2 ** 31 - 1]
    with pytest.raises(ValueError, match=">= 0"):
        mk.Dictionary([1, -2], [1, 1], [1, 1])
    with pytest.raises(ValueError, match="one entry per index"):
        mk.Dictionary([1, 2], [1], [1, 1])


@pytest.mark.parametrize("off", [[1, 3], [0, 2], [0, 4], [0, 2, 1, 3], [], [[0, 3]]])
def test_offsets_that_do_not_rise_from_0_to_n_are_refused(off):
    with pytest.raises(ValueError, match="doc_offsets"):
        mk.host_offsets(np.array(off, np.int64), 3)
    with pytest.raises(ValueError, match="doc_offsets"):
        mk.host_offsets(torch.tensor(off, dtype=torch.int64), 3)


def test_good_offsets_pass():
    assert mk.host_offsets([0, 0, 3, 3], 3).tolist() == [0, 0, 3, 3] and mk.host_offsets([0], 0).tolist() == [0]


@pytest.mark.parametrize("bucket", [[0, 65536, 1], [0, -1, 1], [0, 1], [0, 1, 2, 3]])
def test_oov_bucket_outside_its_range_is_refused(bucket):
    with pytest.raises(ValueError, match="oov_bucket"):
        mk.check_host_buckets(bucket, 3)


def test_good_buckets_pass():
    assert mk.check_host_buckets([0, 65535, 7], 3).dtype == np.int32

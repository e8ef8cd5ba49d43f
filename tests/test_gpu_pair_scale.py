"""GPU: the pair-table builders, the neighbour table and the item-kNN recommender ABOVE ONE LAUNCH GRID.

esr_cooccur.hip, esr_dice.hip, esr_terms.hip and esr_neighbours.hip size every grid with grid_for or min(kMaxGrid, ...):
2048 workgroups of 256 threads.  Above GRID_ELEMS = 524 288 elements (GRID_WAVES = 8 192 items for the one-wave-per-item
kernels, 2 048 items for the one-workgroup-per-item kernels) a kernel goes round its grid-stride loop, and other paths
wake up with it: a second round of positions, a scan carry, LDS reused by a workgroup's second item.  The other tests of
these stages stay far below that; here every input is the smallest that crosses the threshold its case is named for, and
every case asserts ON THE HOST, before any launch, that it does.

Every comparison is torch.equal / np.array_equal on every output array against the vectorised oracles of
tests/_pair_scale_ref.py (test_pair_scale_ref.py holds those bit for bit against the pure-Python restatements).  Inputs and
oracles are built once per module.  Each docstring names the paths its case reaches and why a broken stride, carry or
LDS hand-over there could not pass."""
import functools

import numpy as np
import pytest
import torch

import _pair_scale_ref as ps
from _neighbours_ref import ref_recommend
from _pair_scale_ref import GRID_BLOCKS, GRID_ELEMS, GRID_WAVES
from esrecsys_amd.wikipedia import count_terms as ct
from esrecsys_amd.wikipedia import make_cooccurrence as mc
from esrecsys_amd.wikipedia import make_dice as md
from esrecsys_amd.wikipedia import make_dictionary as mk
from esrecsys_amd.wikipedia import neighbours as nbm
from test_gpu_itemknn import WIDTH, device_table, host_table

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 2


def _frozen(arrays):
    for x in arrays:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return arrays


def _equal(got, want, names):
    """torch.equal of every device tensor with its oracle array, cast to the tensor's dtype only where the oracle's ids are
    int64 and the values fit."""
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        w = np.ascontiguousarray(w)
        assert tuple(g.shape) == w.shape, (name, tuple(g.shape), w.shape)
        if w.dtype == np.int64 and g.dtype == torch.int32:
            assert w.size == 0 or (-1 <= w.min() and w.max() < 2 ** 31), name          # (-1: outside the dictionary)
            w = w.astype(np.int32)
        assert g.dtype == torch.from_numpy(w).dtype, (name, g.dtype, w.dtype)
        assert torch.equal(g.cpu(), torch.from_numpy(w)), name


# ---- co-occurrence ------------------------------------------------------------------------------------------------------
COOCCUR_W, COOCCUR_CALL = 3, 600_000


@functools.lru_cache(maxsize=None)
def cooccur_corpus():
    """Two calls of 600 000 tokens, ids uniform over 20 000, documents of 0..400 tokens with empty ones among them.  Call 0:
    one document straddles token 524 288.  Call 1: a document boundary sits exactly at 524 288."""
    rng = np.random.default_rng(41)
    calls = []
    for c in range(2):
        tokens = rng.integers(0, 20_000, COOCCUR_CALL).astype(np.int32)
        cuts = np.sort(rng.integers(0, COOCCUR_CALL + 1, 3000))           # repeated cuts are empty documents
        cuts = cuts[(cuts < GRID_ELEMS - 150) | (cuts > GRID_ELEMS + 150)]
        if c == 1:
            cuts = np.sort(np.concatenate([cuts, [GRID_ELEMS, GRID_ELEMS]]))     # and an empty document at the boundary
        offsets = np.concatenate([[0, 0], cuts, [COOCCUR_CALL, COOCCUR_CALL]]).astype(np.int64)
        calls.append(_frozen((tokens, offsets)))
    return tuple(calls)


@functools.lru_cache(maxsize=None)
def cooccur_oracle():
    (t0, o0), (t1, o1) = cooccur_corpus()
    return _frozen(ps.vec_cooccur(np.concatenate([t0, t1]), np.concatenate([o0, o1[1:] + t0.size]), COOCCUR_W))


def test_cooccur_two_rounds_growth_and_a_strided_finalize(dev):
    """Reaches: rounds = 2 in cooccur_accumulate_kernel (600 000 positions over 2048 x 256 lanes; drop the `r *` term of
    the position and round 1 repeats positions 0..75 711 instead of taking 524 288..599 999: their pairs are missing and
    the first ones double); cooccur_rehash_kernel over a source of 2^21 and then 2^22 slots, cooccur_init_kernel and
    cooccur_compact_kernel over 2^23 (a lost `+= gridDim.x` stride leaves the slots above 524 288 behind: pairs vanish);
    esr_segment_sort_ids, cooccur_gather_kernel and cooccur_emit_kernel over nnz > 524 288 entries (without their
    stride the output above entry 524 288 is never written: torch.equal on index, other and count sees it).
    Host-side proof: the asserts on COOCCUR_CALL, the straddling document, the boundary, the growth and nnz below."""
    (t0, o0), (t1, o1) = cooccur_corpus()
    assert COOCCUR_CALL > GRID_ELEMS and 2 * GRID_ELEMS > COOCCUR_CALL                       # rounds == 2, in one launch
    d = int(np.searchsorted(o0, GRID_ELEMS, side="right")) - 1
    assert o0[d] < GRID_ELEMS - 3 and o0[d + 1] > GRID_ELEMS + 3                              # a window crosses the round
    assert GRID_ELEMS in o1 and (np.diff(o0) == 0).sum() > 3 and (np.diff(o1) == 0).sum() > 3
    ei, eo, ec = cooccur_oracle()
    assert len(ei) > GRID_ELEMS
    b = mc.CooccurrenceBuilder(COOCCUR_W, capacity=1 << 10, device=dev)
    assert b.max_pairs_per_launch >= COOCCUR_CALL * COOCCUR_W                                 # one launch per add
    b.add(t0, o0)
    first = (b.rehashes, b.capacity)
    assert first[0] >= 1 and first[1] // 2 > GRID_ELEMS           # settle doubled a table of more than GRID_ELEMS slots
    b.add(t1, o1)
    assert b.rehashes > first[0] and b.capacity > first[1] and b.capacity // 2 > GRID_ELEMS  # the table grew twice
    assert b.nnz == len(ei) > GRID_ELEMS
    whole = b.finalize()
    _equal(whole, (ei, eo, ec), ("index", "other", "count"))
    # the same corpus in launches below the threshold: the result must not depend on the cut
    small = mc.CooccurrenceBuilder(COOCCUR_W, capacity=1 << 10, device=dev, max_pairs_per_launch=COOCCUR_W * 100_000)
    assert small.max_pairs_per_launch // COOCCUR_W < GRID_ELEMS
    small.add(t0, o0).add(t1, o1)
    for x, y in zip(small.finalize(), whole):
        assert torch.equal(x, y)


# ---- term stages --------------------------------------------------------------------------------------------------------
TERMS_DICT = 550_000


def _sparse(x):
    """Dense draws -> sparse ids in [0, 2^31 - 1] (an odd multiplier: distinct draws stay distinct)."""
    return ((np.asarray(x, np.int64) * 2654435761 + 12345) % (1 << 31)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def terms_corpus():
    """1.2 M tokens in about 9 000 documents: 560 000 ids that occur once, Zipf draws over 30 000 more (hot ids, repeats
    inside a document, frequency ties everywhere), ids 0 and 2^31 - 1 among them; empty documents."""
    rng = np.random.default_rng(43)
    dense = np.concatenate([np.arange(40_000, 600_000), 1 + (rng.zipf(1.2, 640_000) - 1) % 30_000])
    tokens = _sparse(rng.permutation(dense))
    tokens[[5, 70_000, 1_100_000]] = [0, 2 ** 31 - 1, 2 ** 31 - 1]
    cuts = np.sort(rng.integers(0, tokens.size + 1, 9000))
    offsets = np.concatenate([[0, 0], cuts, [tokens.size]]).astype(np.int64)
    return _frozen((tokens, offsets))


@functools.lru_cache(maxsize=None)
def terms_oracle():
    tokens, offsets = terms_corpus()
    stats = ps.vec_stats(tokens, offsets)
    dictionary = ps.vec_dictionary(*stats, min_frequency=1, max_size=TERMS_DICT)
    return _frozen(stats), _frozen(dictionary)


@pytest.fixture(scope="module")
def terms_dictionary(dev):
    """The statistics and the dictionary from the device, made once; test_terms_statistics_and_dictionary checks them."""
    tokens, offsets = terms_corpus()
    assert GRID_ELEMS < tokens.size <= 1 << 21                                                # one launch, three rounds
    builder = mk.TermStatsBuilder(capacity=1 << 10, device=dev).add(tokens, offsets)
    stats = builder.finalize()
    return builder, stats, mk.make_token_dictionary(*stats, min_frequency=1, max_size=TERMS_DICT)


def test_terms_statistics_and_dictionary(dev, terms_dictionary):
    """Reaches: rounds = 3 in terms_accumulate_kernel (1.2 M tokens in ONE launch; without the `r *` term of the position
    two thirds of the tokens are never counted); terms_fold_kernel over a scratch table of 2^22 slots and
    terms_stats_kernel over a persistent table of 2^22 slots holding more than 524 288 ids (a lost `+= gridDim.x` stride
    drops every id whose slot is above 524 288); esr_segment_sort_ids over K > 524 288 ids up to 2^31 - 1.
    Host-side proof: the asserts on the token count, the single launch, the capacities and the id count below."""
    builder, stats, dictionary = terms_dictionary
    tokens, offsets = terms_corpus()
    (e_ids, e_frequency, e_df), e_dict = terms_oracle()
    assert len(e_ids) > GRID_ELEMS and e_ids[0] == 0 and e_ids[-1] == 2 ** 31 - 1
    assert builder.launches == 1 and builder.capacity > GRID_ELEMS and builder.num_ids == len(e_ids)
    assert mk.pow2_at_least(2 * tokens.size) > GRID_ELEMS                                     # the scratch table's slots
    _equal(stats, (e_ids, e_frequency, e_df), ("ids", "frequency", "doc_frequency"))
    # the dictionary: more than 524 288 entries, cut at max_size inside the tie of the ids that occur once
    assert len(e_dict[0]) == TERMS_DICT > GRID_ELEMS and e_dict[1][-1] == 1 and len(e_ids) > TERMS_DICT + 1000
    _equal((dictionary.ids, dictionary.frequency, dictionary.doc_frequency), e_dict, ("ids", "frequency", "doc_frequency"))
    assert dictionary.max_doc_frequency == int(e_dict[2].max())


def test_terms_lookup_of_every_token(dev, terms_dictionary):
    """Reaches: terms_lookup_build_kernel over K = 550 000 keys and terms_lookup_kernel over N > 524 288 tokens (a lost
    stride leaves dictionary ids unfindable, or output words unwritten).  Tokens inside the dictionary, the 36 000 the
    cut left outside, ids that never occurred, and 0 / 65535 / 65536 / 2^31 - 2 / 2^31 - 1.
    Host-side proof: the asserts on K, N and the outside share below."""
    _builder, _stats, dictionary = terms_dictionary
    tokens, _ = terms_corpus()
    rng = np.random.default_rng(47)
    tokens = np.concatenate([tokens, np.array([0, 65535, 65536, BIG, BIG + 1], np.int32),
                             rng.integers(0, BIG, 5000).astype(np.int32)])
    buckets = rng.integers(0, 65536, tokens.size).astype(np.int32)
    e_dict = terms_oracle()[1]
    e_index, e_default = ps.vec_embedding(tokens, e_dict[0])
    _, e_bucket = ps.vec_embedding(tokens, e_dict[0], buckets)
    assert dictionary.size > GRID_ELEMS and tokens.size > GRID_ELEMS
    assert 0.01 < (e_index < 0).mean() < 0.5 and (e_index[-5000:] < 0).sum() > 4900
    dev_tokens = torch.from_numpy(tokens).to(dev)
    _equal((dictionary.index_of(dev_tokens), dictionary.embedding_indices(dev_tokens),
            dictionary.embedding_indices(dev_tokens, torch.from_numpy(buckets).to(dev))),
           (e_index, e_default, e_bucket), ("index_of", "embedding_indices", "embedding_indices with buckets"))


def test_terms_tfidf_rows(dev, terms_dictionary):
    """Reaches: terms_tfidf_rows_kernel over more than 8 192 rows (one wave per row: a lost stride leaves the rows above
    8 192 unwritten), the accumulate kernel with a lookup table in three rounds, and esr_cooccur_finalize (compact, two
    sorts, gather, emit) over more than 524 288 (document, index) entries with num_ids = K > 524 288.  Stopwords go
    through the lookup table's skip list.
    The norm's fp64 sum runs in the kernel's own order (ps.wave_norm: lane-strided, then a butterfly), so this comparison
    is bit for bit where test_gpu_terms.py, against insertion order, allows 1 ulp.
    Host-side proof: the asserts on the rows and the entries below."""
    _builder, _stats, dictionary = terms_dictionary
    tokens, offsets = terms_corpus()
    e_dict = terms_oracle()[1]
    stop = (int(e_dict[0][0]), int(e_dict[0][1]), int(e_dict[0][2]), 123456789)
    want = ps.vec_sparse_docs(tokens, offsets, e_dict[0], e_dict[2], int(e_dict[2].max()), stop, "wave")
    rows = np.diff(want[0])
    assert offsets.size - 1 > GRID_WAVES and want[1].size > GRID_ELEMS
    assert (rows == 0).sum() > 2 and rows.max() > 2 * 64 and (rows[GRID_WAVES:] > 0).sum() > 500
    builder = ct.TfidfBuilder(dictionary, stopwords=stop, device=dev)
    got = builder.transform(tokens, offsets)
    assert builder.launches == 1
    _equal(got, want, ("out_offsets", "token_index", "token_tfidf"))


# ---- dice ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dice_corpus():
    """8 300 documents of 0..64 ids (the wave path; Zipf draws, so ids repeat inside a document), 2 100 of 65..100 ids (one
    triangle tile each), one of 1 000 ids (16 tiles) and one of exactly 4 096 distinct ids (256 tiles), shuffled; all ids
    below 20 000, so the long documents share theirs with the rest."""
    rng = np.random.default_rng(53)
    short = np.where(rng.random(8300) < 0.7, rng.integers(0, 9, 8300), rng.integers(9, 65, 8300))
    short[:6] = [0, 0, 1, 63, 64, 64]
    docs = [((rng.zipf(1.2, int(n)) - 1) % 20_000).astype(np.int32) for n in short]
    for n in rng.integers(65, 101, 2100):
        doc = rng.integers(0, 20_000, int(n)).astype(np.int32)
        doc[-3:] = doc[:3]                                                # repeats inside a long document too
        docs.append(doc)
    docs.append(rng.integers(0, 20_000, 1000).astype(np.int32))
    docs.append(rng.choice(20_000, md.MAX_DOC, replace=False).astype(np.int32))
    docs = [docs[i] for i in rng.permutation(len(docs))]
    return _frozen(md.pack_docs(docs))


@functools.lru_cache(maxsize=None)
def dice_oracle():
    return _frozen(ps.vec_dice(*dice_corpus()))


def test_dice_strided_waves_and_a_work_list_above_the_grid(dev):
    """Reaches: dice_small_kernel over more than 8 192 documents (one wave per document: a lost stride drops the documents
    above 8 192); dice_large_kernel with more than 2 048 work items, so workgroups take a second and third (document,
    tile) item -- a one-tile document after a tile of the 4 096-id document and the reverse -- and reuse s, s_cnt and s_u
    behind the loop-head __syncthreads() (without it a fast wave loads the next document into s while a slow one still
    emits pairs from the last: wrong keys, which no longer sum to the oracle's counts); table init, rehash source and
    compact over millions of slots, finalize over more than 16 M entries.
    Host-side proof: the asserts on the document count, the work-list length and its composition below."""
    tokens, offsets = dice_corpus()
    n = np.diff(offsets)
    tiles = np.where(n > 64, -(-(n * (n - 1) // 2) // 32768), 0)
    assert n.size > GRID_WAVES and (n[GRID_WAVES:] > 0).sum() > 1000 and (n == 0).sum() > 100
    assert tiles.sum() > GRID_BLOCKS and sorted(tiles[tiles > 1].tolist()) == [16, 256] and (tiles == 1).sum() == 2100
    assert n.max() == md.MAX_DOC and np.sort(n)[-3] <= 100
    index, other, count, ids, df = dice_oracle()
    assert 12_000_000 < len(index) < 40_000_000 and count.max() > 3
    builder = md.DiceBuilder(capacity=1 << 12, device=dev)
    builder.add(tokens, offsets)
    assert builder.launches == 1
    _equal(builder.finalize() + builder.doc_frequency(), (index, other, count, ids, df),
           ("index", "other", "count", "ids", "df"))


# ---- neighbours: more than 524 288 ids and entries ----------------------------------------------------------------------
NB_U = 530_000
NB_CLASSES = ((0, 0), (1, 16), (17, 64), (65, 70))       # empty, packed wave, wave, workgroup: (shortest, longest) row


@functools.lru_cache(maxsize=None)
def big_table():
    """(index, other, count, ids, df, hub_rows, hub_lengths).  530 000 sparse ids.  HUB rows sit in 3 584 quads of four
    consecutive rows scattered over the id range -- the 256 ways to fill a quad from NB_CLASSES, 14 times each -- plus 40
    streaming rows of 2 049..7 000 entries; the last row is a hub.  Partners come from a pool of 60 000 other ids, so in
    the stored orientation a hub's row has exactly its length and most rows are empty; in both orientations the pool's
    rows hold the hubs that chose them.  Small integer counts and document frequencies: scores tie at every k."""
    rng = np.random.default_rng(59)
    ids = np.unique(np.concatenate([rng.integers(0, BIG, NB_U + 2000), [0, BIG]]))[-NB_U:].astype(np.int64)
    assert ids.size == NB_U and ids[-1] == BIG
    nquads = NB_U // 4
    quads = np.concatenate([rng.choice(nquads - 1, 14 * 256 - 1, replace=False), [nquads - 1]])
    patterns = np.tile(np.arange(256), 14)
    cls = (patterns[:, None] >> (2 * np.arange(4))) & 3                  # [quad, position] -> class
    lo, hi = np.array(NB_CLASSES)[cls, 0], np.array(NB_CLASSES)[cls, 1]
    lengths = np.zeros(NB_U, np.int64)
    lengths[(4 * quads[:, None] + np.arange(4)).reshape(-1)] = rng.integers(lo, hi + 1).reshape(-1)
    lengths[NB_U - 1] = max(lengths[NB_U - 1], 7)                         # the row that writes offsets[u]
    free = np.setdiff1d(np.arange(NB_U), (4 * quads[:, None] + np.arange(4)).reshape(-1))
    free = rng.permutation(free)
    stream = free[:40]
    lengths[stream] = np.concatenate([[2049, 7000], rng.integers(2049, 7001, 38)])
    pool = np.sort(free[40:60_040])
    hub_rows = np.flatnonzero(lengths)
    hub = np.repeat(hub_rows, lengths[hub_rows])
    partner = np.concatenate([rng.choice(pool, int(n), replace=False) for n in lengths[hub_rows]])
    count = rng.integers(1, 6, hub.size).astype(np.float32)
    df = rng.integers(1, 5, NB_U).astype(np.float32)
    order = np.lexsort((partner, hub))
    return _frozen((ids[hub][order], ids[partner][order], count[order], ids, df, hub_rows, lengths[hub_rows]))


@functools.lru_cache(maxsize=None)
def big_ref(orientation, score):
    """The oracle at k = 10, computed once: k = 1 is its first column."""
    index, other, count, ids, df, _rows, _lengths = big_table()
    return _frozen(ps.vec_neighbours(index, other, count, ids, df, 10, orientation, score))


def _cut(ref, k):
    ids, nb, sc, ct, lengths = ref
    return ids, nb[:, :k], sc[:, :k], ct[:, :k], np.minimum(lengths, k).astype(np.int32)


def _device(dev, index, other, count, ids, df):
    t = lambda a, dt: torch.from_numpy(np.asarray(a).astype(dt)).to(dev)  # noqa: E731
    return t(index, np.int32), t(other, np.int32), t(count, np.float32), t(ids, np.int32), t(df, np.float32)


def _table_equal(table, want):
    _equal((table.ids, table.neighbours, table.scores, table.counts, table.lengths), want,
           ("ids", "neighbours", "scores", "counts", "lengths"))


def test_the_big_table_is_over_every_threshold_it_is_named_for():
    """The host-side proof of test_neighbours_above_one_grid, on the input itself (no device)."""
    index, other, _count, ids, _df, hub_rows, hub_lengths = big_table()
    u, nnz = ids.size, index.size
    assert nnz > GRID_ELEMS                                        # degree, fill: the entry loops stride
    assert u > GRID_ELEMS                                          # pad strides; -(-u // 2048) scan tiles:
    assert -(-u // 2048) == 259 > 256                              # nb_tile_scan_kernel's carry loop runs twice
    assert -(-u // 4) > GRID_WAVES                                 # nb_select_wave_kernel walks more than 8 192 quads
    assert hub_rows[-1] == u - 1 and (hub_rows < GRID_ELEMS).sum() > 10_000 and (hub_rows >= GRID_ELEMS).sum() > 50
    assert hub_rows.size < u // 20                                 # most rows are empty
    stored = np.bincount(np.searchsorted(ids, index), minlength=u)
    assert np.array_equal(stored[hub_rows], hub_lengths) and stored.sum() == nnz      # a hub is nobody's partner
    both = stored + np.bincount(np.searchsorted(ids, other), minlength=u)
    for rows in (stored, both):
        long_rows = (rows > 64).sum()
        assert long_rows > GRID_BLOCKS                             # nb_select_block_kernel: second rows per workgroup
        assert ((rows > 64) & (rows <= 2048)).sum() > 2100 and (rows > 2048).sum() == 40
        assert {2049, 7000} <= set(rows[rows > 2048].tolist())
    # every way to fill a quad from (empty, <= 16, 17..64, 65..70) occurs, on both sides of the first grid round of quads
    cls = np.searchsorted([1, 17, 65], stored, side="right").reshape(-1, 4)
    code = (cls * 4 ** np.arange(4)).sum(1)
    assert np.unique(code[code > 0]).size == 255 and np.unique(code[GRID_WAVES:][code[GRID_WAVES:] > 0]).size == 255


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("score", ["dice", "count"])
@pytest.mark.parametrize("orientation", ["stored", "both"])
def test_neighbours_above_one_grid(dev, orientation, score, k):
    """Reaches: nb_pad_kernel over u k words (k = 10; without its `+= gridDim.x` stride the padding above word 524 288
    is not -1 / 0), nb_degree_kernel and nb_fill_kernel over nnz > 524 288 entries, ids looked up among 530 000 (without
    theirs the entries above 524 288 -- sorted by row, so the upper rows' -- are never counted or placed: lengths and
    partners differ); nb_tile_sums_kernel and nb_offsets_kernel over 259 scan tiles; nb_tile_scan_kernel's second batch
    of 256 tiles -- drop its `carry +=` line and tiles 256..258 restart from 0: the offsets of rows 524 288.. fall into
    the first rows' entries, and the hubs up there (the last row among them, which also writes offsets[u]) come out with
    other rows' partners; nb_select_wave_kernel over 132 500 quads (more than 8 192: without its stride every row from
    32 768 on stays padding), all 255 quad mixes of empty / packed / wave / long rows on the strided side too;
    nb_select_block_kernel with 3 600 listed rows on 2 048 workgroups: the first 1 500 workgroups take a second row, and
    as the 40 streaming rows are spread over the list (its order is the atomics'), workgroup-class rows follow streaming
    rows and the reverse.  s_key / s_pay / s_hist / s_n are reused behind the loop-head __syncthreads(): without it a
    wave that is still emitting row one reads keys that another wave has loaded for row two.
    Host-side proof: test_the_big_table_is_over_every_threshold_it_is_named_for."""
    index, other, count, ids, df, _rows, _lengths = big_table()
    assert index.size > GRID_ELEMS and ids.size > GRID_ELEMS
    d_index, d_other, d_count, d_ids, d_df = _device(dev, index, other, count, ids, df)
    table = nbm.neighbours(d_index, d_other, d_count, d_ids, d_df if score == "dice" else None, k, orientation, score)
    _table_equal(table, _cut(big_ref(orientation, score), k))


# ---- neighbours: the streaming select on real scores --------------------------------------------------------------------
STREAM_KS = [1, 64, 1024]
STREAM_ROWS = (2049, 5000, 7000)


@functools.lru_cache(maxsize=None)
def stream_table():
    """Three rows of 2 049, 5 000 and 7 000 entries (ids 0, 1, 2) over a pool of 7 400 partner ids.  Counts are
    full-mantissa float32 values over 40 binades; sorted by score, the entries at positions 0..4, 58..71 and 1 010..1 039
    of every row share ONE count (so the tie straddles k = 1, 64 and 1 024 and the partner id in the key's low 32 bits
    decides), and the last 20 are 0.  The pool holds ids whose low byte, and low two bytes, are 0x00 and 0xFF.
    df = 2 everywhere: a dice score is count / 4, which keeps every tie."""
    rng = np.random.default_rng(61)
    m = np.arange(1, 1200, dtype=np.int64)
    pool = np.unique(np.concatenate([256 * m + 1024, 256 * m + 1024 + 255, 65536 * m, 65536 * m + 65535,
                                     [BIG, BIG - 1, 255, 256]]))
    pool = np.sort(np.concatenate([pool, np.setdiff1d(rng.integers(3, BIG, 4000), pool)[:7400 - pool.size]]))
    assert pool.size == 7400 and pool[-1] == BIG and pool[0] > 2
    hub, partner, count = [], [], []
    for h, n in enumerate(STREAM_ROWS):
        c = np.sort((rng.random(n, dtype=np.float32) * np.float32(2.0) ** rng.integers(-20, 20, n)).astype(np.float32))[::-1]
        for a, b in ((0, 5), (58, 72), (1010, 1040)):
            c[a:b] = c[a]
        c[-20:] = 0
        hub.append(np.full(n, h, np.int64))
        partner.append(rng.choice(pool, n, replace=False))                # (the sorted scores meet the partners in random order)
        count.append(c.copy())
    hub, partner, count = np.concatenate(hub), np.concatenate(partner), np.concatenate(count)
    order = np.lexsort((partner, hub))
    ids = np.concatenate([[0, 1, 2], pool])
    return _frozen((hub[order], partner[order], count[order], ids, np.full(ids.size, 2, np.float32)))


@functools.lru_cache(maxsize=None)
def stream_ref(score):
    return _frozen(ps.vec_neighbours(*stream_table(), 1024, "both", score))


def test_the_streaming_table_holds_what_it_is_for():
    """Host-side proof of test_streaming_select_on_real_scores: the rows are of the streaming class, every byte of the
    score bits takes many values, every k is straddled by a tie that the partner id decides, zeros and the 0x00 / 0xFF
    bytes are there."""
    index, other, count, ids, _df = stream_table()
    assert nbm.plan_bounds()[-1] == 2048 and tuple(np.bincount(index)) == STREAM_ROWS and min(STREAM_ROWS) > 2048
    bits = count.view(np.uint32)
    digits = [np.unique((bits >> (8 * b)) & 255).size for b in range(4)]
    assert min(digits[:3]) >= 250 and digits[3] >= 12 and (count == 0).sum() == 60
    low = other & 255
    assert (low == 0).sum() > 500 and (low == 255).sum() > 500 and ((other & 0xFFFF) == 0xFFFF).sum() > 100
    for score in ("count", "dice"):
        _ids, nb, sc, _ct, lengths = stream_ref(score)
        assert lengths[:3].tolist() == [1024] * 3 and lengths[3:].max() <= 3
        for r in range(3):
            mine = index == r
            row = np.sort(count[mine])[::-1]
            for k in STREAM_KS:
                assert row[k - 1] == row[k] and sc[r, k - 1] == row[k] / np.float32(1 if score == "count" else 4)
                above = int((row > row[k]).sum())                                         # the tie straddles position k,
                tied = np.sort(other[mine & (count == row[k])])                           # and its lowest ids win
                assert above < k < above + tied.size and np.array_equal(nb[r, above:k], tied[:k - above])


@pytest.mark.parametrize("k", STREAM_KS)
@pytest.mark.parametrize("score", ["count", "dice"])
def test_streaming_select_on_real_scores(dev, score, k):
    """Reaches: the 8-pass radix select of nb_select_block_kernel on keys that differ in every byte -- every pass meets
    many occupied digits, not the two or three that small integer scores leave -- with the k-th key inside a group of
    equal score bits, so passes 3..0 (the partner id) pick it, through digits 0x00 and 0xFF; counts of 0 (the key's
    largest score digit); three streaming rows of which two share no workgroup.
    Host-side proof: test_the_streaming_table_holds_what_it_is_for."""
    host = stream_table()
    assert all(n > nbm.plan_bounds()[-1] for n in STREAM_ROWS)
    index, other, count, ids, df = _device(dev, *host)
    table = nbm.neighbours(index, other, count, ids, df if score == "dice" else None, k, "both", score)
    _table_equal(table, _cut(stream_ref(score), k))


# ---- recommender --------------------------------------------------------------------------------------------------------
RECOMMEND_QUERIES = 2100


@functools.lru_cache(maxsize=None)
def recommend_queries():
    """2 100 queries over test_gpu_itemknn's table: history lengths from 0 up to the cap (128 ids at width 16), mostly
    short; query q and query q + 2048 -- one workgroup's first and second -- always differ in length, with the cap after
    an empty one, an empty one after the cap and every step between.  A tenth of the ids are unknown to the table, the
    last id of a history repeats its first."""
    rng = np.random.default_rng(67)
    full = nbm.max_entries() // WIDTH
    lengths = np.where(rng.random(RECOMMEND_QUERIES) < 0.85, rng.integers(0, 12, RECOMMEND_QUERIES),
                       rng.integers(12, full + 1, RECOMMEND_QUERIES))
    second = RECOMMEND_QUERIES - GRID_BLOCKS
    lengths[:second] = np.resize([0, full, 1, full, 5, 0, 40, 2, full - 1, 3], second)
    lengths[GRID_BLOCKS:] = np.resize([full, 0, full, 1, 0, 5, 2, 40, 3, full - 1], second)
    ids = host_table()[0]
    history = []
    for n in lengths:
        h = rng.choice(ids, int(n)).astype(np.int64)
        h[rng.random(int(n)) < 0.1] = rng.integers(0, BIG)
        if n >= 3:
            h[n - 1] = h[0]
        history.append(h)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return _frozen((np.concatenate(history).astype(np.int32), offsets))


@pytest.mark.parametrize("exclude", [True, False], ids=["exclude_history", "keep_history"])
def test_recommend_second_queries_per_workgroup(dev, exclude):
    """Reaches: itemknn_recommend_kernel with nq = 2 100 > 2 048 workgroups: workgroups 0..51 take a second query, of
    another length than their first (so another sort size m over the same s_key / s_val / s_hist / s_cnt), behind the
    loop-head __syncthreads() -- without it the second query's gather overwrites s_key while a slow wave still emits the
    first query's winners, and s_cnt is reset under its readers.  A lost `+= gridDim.x` leaves queries 2 048.. unwritten.
    Host-side proof: the asserts on nq and the paired lengths below."""
    history, offsets = recommend_queries()
    lengths = np.diff(offsets)
    full = nbm.max_entries() // WIDTH
    assert lengths.size == RECOMMEND_QUERIES > GRID_BLOCKS and lengths.min() == 0 and lengths.max() == full
    pairs = list(zip(lengths[:RECOMMEND_QUERIES - GRID_BLOCKS].tolist(), lengths[GRID_BLOCKS:].tolist()))
    assert all(a != b for a, b in pairs) and {(0, full), (full, 0), (1, full), (full - 1, 3)} <= set(pairs)
    want = ref_recommend(host_table(), history, offsets, 50, exclude_history=exclude)
    assert (want[2][GRID_BLOCKS:] > 0).sum() > 25 and want[2].max() == 50 and (want[2] == 0).sum() > 50
    got = nbm.recommend(device_table(dev), torch.from_numpy(history).to(dev), offsets, 50, exclude_history=exclude)
    _equal(got, want, ("ids", "scores", "lengths"))

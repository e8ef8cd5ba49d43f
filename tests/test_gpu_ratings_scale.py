"""GPU: the user-similarity table and the user-kNN predictor (esr_ratings.hip, esrecsys_amd/ratings.py) past one tile, one
wave and one launch grid, bit for bit against the CPU oracle tests/_ratings_ref.py (integers by array_equal, float32
through uint32 views; no tolerance anywhere).  tests/test_gpu_ratings.py covers the small geometry; here every input is
over a threshold of the kernels, and every test asserts that ON THE HOST, before the device is touched, from the library's
own constants: a later change of a constant fails the test instead of leaving it testing nothing.

  finalize    usersim_tile_scan_kernel carries a sum over rounds of kBlock tiles of kBlock rows (nnz > 65 536);
              usersim_score / usersim_emit stride over tiles above kMaxGrid of them (nnz > 524 288); usersim_init /
              usersim_rehash / usersim_compact stride over slots above kMaxGrid * kBlock of them.
  accumulate  tile_decode with cq up to 16, interior tiles (cp < cq), a last chunk that is not full.
  predict     rows of several 64-column chunks (one ballot / shuffle fold per chunk, carried in one accumulator, in
              ascending column order: the order witness makes that order visible in float32), knn_den_all over a long row,
              more queries than the grid has waves.
  recommend   widths up to kUserKnnMaxWidth at the cap of gathered ratings, runs of empty columns in s_start, second
              queries per workgroup that reuse s_key / s_val / s_cnt / s_den.
"""
import functools

import numpy as np
import pytest
import torch

from _ratings_ref import RefUserKnn, vec_similarity
from esrecsys_amd import ops
from esrecsys_amd import ratings as rt
from esrecsys_amd.wikipedia import neighbours as nbm
from esrecsys_amd.wikipedia.pair_table import pow2_at_least
from test_gpu_ratings import BIG, MODES, assert_sim, build, frozen, small_corpus, small_models, to_dev

pytestmark = pytest.mark.gpu

BLOCK = 256                      # esr_common.h kBlock: threads per workgroup, rows per finalize tile
MAX_GRID = 256 * 8               # esr_common.h kMaxGrid, as test_gpu_evaluate.py states it
GRID_ELEMS = MAX_GRID * BLOCK    # one element per thread: a loop over more strides
GRID_WAVES = MAX_GRID * 4        # one query (one tile) per wave
WAVE = 64                        # the columns of a table row that one fold of the predict kernel takes
MAX_WIDTH = 1024                 # kUserKnnMaxWidth = neighbours.MAX_K


def T():
    return ops.usersim_tile()


def user_pool(rng, n):
    """n distinct user ids, sparse over [1000, 2^31 - 2], the largest one among them; in random order."""
    ids = np.unique(rng.integers(1000, BIG, n + 64))
    return rng.permutation(np.append(rng.choice(ids[ids < BIG], n - 1, replace=False), BIG)).astype(np.int64)


def rows_of(rng, items):
    """(user, item, dev) shuffled, from [(item id, its raters)]: deviations of both signs."""
    user = np.concatenate([u for _i, u in items])
    item = np.concatenate([np.full(u.size, i, np.int64) for i, u in items])
    dev = rng.integers(-5000, 5001, user.size)
    p = rng.permutation(user.size)
    return frozen(user[p], item[p], dev[p])


def stored(want):
    """The entries the table holds for an oracle without filters: the kept rows and the flat ones."""
    return want[0].size + want[4]


# ---- similarity: the scan carry --------------------------------------------------------------------------------------
CARRY_N, CARRY_SECOND = 400, 70


@functools.lru_cache(maxsize=None)
def carry_rows():
    """Item 0: 400 raters.  Item 1: 70 of them (those pairs meet twice).  Items 2, 3, 5, 8: one rater each -- no pair; by
    item id modulo 3 (``build(adds=3)``) the adds hold items {0, 3}, {1} and {2, 5, 8}: the third only one-rater items."""
    rng = np.random.default_rng(41)
    pool = user_pool(rng, CARRY_N)
    items = [(0, pool), (1, rng.choice(pool, CARRY_SECOND, replace=False))]
    items += [(i, rng.choice(pool, 1)) for i in (2, 3, 5, 8)]
    return rows_of(rng, items)


@functools.lru_cache(maxsize=None)
def carry_ref(min_overlap=1, min_similarity=None):
    out = vec_similarity(*carry_rows(), min_overlap, min_similarity)
    return frozen(*out[:4]) + (out[4],)


def assert_the_carry_case_is_over_its_thresholds():
    t = T()
    user, item, dev = carry_rows()
    want = carry_ref()
    pairs = CARRY_N * (CARRY_N - 1) // 2
    assert stored(want) == pairs == 79_800 > BLOCK * BLOCK            # more than kBlock finalize tiles:
    assert -(-stored(want) // BLOCK) > BLOCK                          # the tile scan goes round its loop twice
    chunks = -(-CARRY_N // t)
    assert chunks == 7 and CARRY_N % t == 16                          # tile_decode up to cq = 6; a last chunk of 16 raters
    assert int(rt.UserSimilarityBuilder.tiles_of(np.array([CARRY_N]), t)[0]) == 28
    assert user.max() == BIG and (dev < 0).sum() > 100 and (dev > 0).sum() > 100
    assert want[3].max() == 2 and (want[3] == 2).sum() == carry_ref(2)[0].size > 2000       # of 70 * 69 / 2 = 2 415
    half = carry_ref(1, 0.0)[0].size                                  # the sign filter keeps about half of the rows:
    assert want[0].size // 4 < half < 3 * want[0].size // 4           # the compaction offsets differ in almost every tile
    kept_per_tile = np.add.reduceat((want[2] > 0).astype(np.int64), np.arange(0, want[0].size, BLOCK))
    assert ((kept_per_tile > 0) & (kept_per_tile < BLOCK)).mean() > 0.9


def test_finalize_carries_its_tile_scan_over_more_than_256_tiles(dev):
    """79 800 entries are 312 finalize tiles: usersim_tile_scan_kernel takes them in two rounds of 256 and the second
    round starts from the first's total.  Without the carry the offsets of tiles 256.. restart from 0 and the upper rows
    overwrite the first ones.  The same table under both filters: ordered compaction over 312 tiles."""
    assert_the_carry_case_is_over_its_thresholds()
    b = build(dev, carry_rows())
    assert b.launches == 1
    assert_sim(b, carry_ref())
    assert_sim(b, carry_ref(1, 0.0), min_similarity=0.0)
    assert_sim(b, carry_ref(2), min_overlap=2)
    assert_sim(b, carry_ref())


def test_division_into_adds_and_launches_at_scale(dev):
    """The same rows in three adds (the third holds only one-rater items: nothing to launch), and with a launch limit
    below the big item's own pair count (an item is never cut: one launch above its bound): the tensors of one add."""
    assert_the_carry_case_is_over_its_thresholds()
    user, item, _dev = carry_rows()
    per_add = [np.unique(item[item % 3 == a]).tolist() for a in range(3)]
    assert per_add == [[0, 3], [1], [2, 5, 8]] and all(np.sum(item == i) == 1 for i in per_add[2])
    b = build(dev, carry_rows(), adds=3)
    assert b.launches == 2
    assert_sim(b, carry_ref())
    assert_sim(b, carry_ref(1, 0.0), min_similarity=0.0)
    assert CARRY_N * (CARRY_N - 1) // 2 > 5000
    b = build(dev, carry_rows(), max_pairs_per_launch=5000)
    assert b.launches == 2                                            # item 0 alone above the limit, then item 1
    assert_sim(b, carry_ref())
    assert_sim(b, carry_ref(2), min_overlap=2)


# ---- similarity: finalize beyond its grid ----------------------------------------------------------------------------
GRID_N = 1030
GRID_MID = (300, 400, 400)       # raters of the items 300, 301, 302: the table grows launch by launch


@functools.lru_cache(maxsize=None)
def grid_rows():
    """Items 0..299: two raters each.  Items 300, 301, 302: 300, 400 and 400 raters.  Item 303: all 1 030 users, so every
    other pair is one of its pairs.  The three middle items are there for the table's growth: ``PairTable.reserve`` goes
    straight to the size a launch needs, so the big item alone would take a table of 2^16 slots to 2^21 in two rehashes;
    with them every launch ends in a doubling and the big item's reserve and settle add two more."""
    rng = np.random.default_rng(43)
    pool = user_pool(rng, GRID_N)
    items = [(i, rng.choice(pool, 2, replace=False)) for i in range(300)]
    items += [(300 + i, rng.choice(pool, n, replace=False)) for i, n in enumerate(GRID_MID)]
    items.append((303, pool))
    return rows_of(rng, items)


@functools.lru_cache(maxsize=None)
def grid_ref(min_similarity=None):
    out = vec_similarity(*grid_rows(), 1, min_similarity)
    return frozen(*out[:4]) + (out[4],)


def test_finalize_beyond_its_grid_after_rehashes_beyond_theirs(dev):
    """529 935 entries: 2 071 finalize tiles on 2 048 workgroups (usersim_score_kernel and usersim_emit_kernel take a
    second tile; the tile scan goes round nine times), compacted out of 2^21 slots (usersim_compact_kernel strides), after a
    last rehash that read 2^20 slots and initialised 2^21 (usersim_rehash_kernel, usersim_init_kernel stride).  The big
    item is 17 chunks = 153 accumulate tiles (tile_decode up to cq = 16, a last chunk of 6 raters) in ONE launch above the
    limit."""
    t = T()
    want = grid_ref()
    big = GRID_N * (GRID_N - 1) // 2
    assert stored(want) == big == 529_935 > GRID_ELEMS                # every other pair is a pair of item 303
    assert -(-stored(want) // BLOCK) > MAX_GRID                       # finalize tiles: score and emit stride
    assert -(-GRID_N // t) == 17 and GRID_N % t == 6
    assert int(rt.UserSimilarityBuilder.tiles_of(np.array([GRID_N]), t)[0]) == 153
    capacity, limit = 1 << 16, 1 << 17
    assert big > limit                                                # the item alone is above the launch limit
    others = 300 + sum(n * (n - 1) // 2 for n in GRID_MID)
    final = pow2_at_least(2 * stored(want))                           # settle: a load factor of at most 1/2
    assert final == 1 << 21 and final // 2 > GRID_ELEMS               # the last rehash reads 2^20 slots: beyond the grid
    assert pow2_at_least(others + big) <= final // 2                  # ... and it IS a doubling: reserve stops below it
    assert want[3].max() >= 3 and want[0].size // 4 < grid_ref(0.0)[0].size < 3 * want[0].size // 4
    b = build(dev, grid_rows(), capacity=capacity, max_pairs_per_launch=limit)
    assert b.launches >= 3 and b.rehashes >= 4 and b.capacity == final
    first = assert_sim(b, want)
    assert_sim(b, grid_ref(0.0), min_similarity=0.0)
    again = b.finalize()
    assert all(torch.equal(x, y) for x, y in zip(first, again)) and b.dropped_flat == want[4]


# ---- hand-made neighbour tables --------------------------------------------------------------------------------------
def signed_sims(rng, n):
    """Full-mantissa float32 similarities over five binades, both signs, none zero."""
    s = (rng.random(n, dtype=np.float32) + np.float32(2.0 ** -20)) * np.float32(2.0) ** rng.integers(-3, 2, n)
    return (s * rng.choice([-1.0, 1.0], n)).astype(np.float32)


class MemoRef(RefUserKnn):
    """The oracle with its affinities kept: ``recommend`` under another k or exclude_rated asks for the same ones."""

    def affinity(self, A, i, center="neighbour", denominator="rated"):
        memo = self.__dict__.setdefault("_memo", {})
        key = (int(A), int(i), center, denominator)
        if key not in memo:
            memo[key] = RefUserKnn.affinity(self, A, i, center, denominator)
        return memo[key]


class World:
    """A neighbour table of width W made on the host, and the ratings under it.  Column j of every row is neighbour j
    (ids in random order, similarities unordered); the four rows have the lengths W, 0, W - 1 and 1.  ``rated[j]`` are the
    items neighbour j rates (half stars); a neighbour with ``in_users[j]`` False is absent from `users` (the kernels'
    pu = -1), one with no items is a user without ratings.  Every query user rates `own`."""

    def __init__(self, W, seed, rated, in_users, own=(0, 3, 6, 9), sims=None):
        rng = np.random.default_rng(seed)
        pool = user_pool(rng, W + 6)
        self.W, self.neighbour, self.rated, self.in_users = W, pool[:W], rated, np.asarray(in_users, bool)
        self.ids = np.sort(pool[W:W + 4]).astype(np.int32)
        self.unknown = int(pool[W + 4])
        self.lengths = np.array([W, 0, W - 1, 1], np.int32)
        nb, sc = np.full((4, W), -1, np.int32), np.zeros((4, W), np.float32)
        for r, n in enumerate(self.lengths):
            nb[r, :n] = self.neighbour[:n]
            sc[r, :n] = signed_sims(rng, n) if sims is None else sims[:n]
        self.table = frozen(self.ids, nb, sc, sc.copy(), self.lengths)
        user = [np.full(len(rated[j]), self.neighbour[j]) for j in range(W) if self.in_users[j]]
        item = [np.asarray(rated[j], np.int64) for j in range(W) if self.in_users[j]]
        user += [np.full(len(own), q) for q in self.ids]
        item += [np.asarray(own, np.int64) for _q in self.ids]
        self.user, self.item = np.concatenate(user).astype(np.int64), np.concatenate(item).astype(np.int64)
        self.rating = rng.integers(1, 11, self.user.size) / 2.0
        self.finish()

    def finish(self):
        """users, mean (the exact float64 sum of half stars / count; 2.5 for a user without ratings) and the oracle."""
        self.users = np.unique(np.concatenate([self.ids, self.neighbour[self.in_users]])).astype(np.int32)
        at = np.searchsorted(self.users, self.user)
        total, count = np.zeros(self.users.size), np.zeros(self.users.size)
        np.add.at(total, at, self.rating), np.add.at(count, at, 1.0)
        self.mean = np.where(count > 0, total / np.maximum(count, 1.0), 2.5)
        self.ref = MemoRef(self.table, self.user, self.item, self.rating, self.users, self.mean)
        return self

    def user_of_length(self, n):
        return int(self.ids[int(np.flatnonzero(self.lengths == n)[0])])

    def counted(self, length, item):
        """The columns of the row of that length whose neighbour rated the item."""
        return [j for j in range(length) if self.in_users[j] and item in self.rated[j]]

    def queries(self):
        return np.append(self.ids.astype(np.int64), self.unknown)


def device_model(dev_, world):
    ids, nb, sc, ct, lengths = (to_dev(dev_, x, x.dtype) for x in world.table)
    table = nbm.NeighbourTable(ids, nb, sc, ct, lengths, "both", "count")
    return rt.UserKnn(table, world.user, world.item, world.rating, world.users, world.mean)


def bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).view(np.uint32)


def assert_predict(model, ref, qu, qi, center, denominator):
    aff, support = model.predict(qu, qi, center, denominator)
    w_aff, w_support = ref.predict(qu, qi, center, denominator)
    assert aff.dtype == torch.float32 and support.dtype == torch.int32
    assert np.array_equal(support.cpu().numpy(), w_support)
    assert np.array_equal(bits(aff), bits(w_aff))
    return w_aff, w_support


def assert_recommend(model, ref, users, k, exclude, min_support, center, denominator):
    got = model.recommend(users, k, exclude, min_support, center, denominator)
    want = ref.recommend(users, k, exclude, min_support, center, denominator)
    assert tuple(got[0].shape) == (len(users), k)
    assert np.array_equal(got[2].cpu().numpy(), want[2])
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    return got, want


# ---- predict across table widths -------------------------------------------------------------------------------------
WIDTHS = [1, 63, 64, 65, 128, MAX_WIDTH]


def marks_of(W):
    return sorted({c for c in (0, WAVE - 1, WAVE, WAVE + 1, W - 1) if c < W})


@functools.lru_cache(maxsize=None)
def width_world(W):
    """Every neighbour rates item 3000 and about a third of the items 0..29; the neighbours of the marked columns (0, 63,
    64, 65, W - 1) also rate item 2000 together and item 1000 + column alone.  Every seventh column, no marked one, is a
    neighbour that `users` lacks."""
    rng = np.random.default_rng(100 + W)
    marks = marks_of(W)
    rated = [np.concatenate([np.flatnonzero(rng.random(30) < 0.3), [3000], [1000 + j, 2000] if j in marks else []])
             .astype(np.int64) for j in range(W)]
    return World(W, 200 + W, rated, [j in marks or j % 7 != 3 for j in range(W)])


def width_items(W):
    return np.array(list(range(0, 30, 3)) + [3000, 2000, 777_777] + [1000 + c for c in marks_of(W)], np.int64)


@pytest.mark.parametrize("W", WIDTHS)
def test_predict_across_table_widths(dev, W):
    """Rows of 0, 1, W - 1 and W columns at widths on both sides of one and two waves and at the cap: the second and later
    64-column chunks of a row, folded into the one accumulator; items counted in column 64 alone, in the last column
    alone, in the columns 63 | 64, 65 across the chunk boundary; knn_den_all over the whole row."""
    assert MAX_WIDTH == nbm.MAX_K and WAVE == T()
    world = width_world(W)
    full = world.user_of_length(W)
    marks = marks_of(W)
    assert set(world.lengths.tolist()) == {0, 1, W - 1, W} and W - 1 in marks
    for c in marks:
        assert world.counted(W, 1000 + c) == [c]                     # counted in that column alone
    assert world.counted(W, 2000) == marks and world.counted(W - 1, 2000) == marks[:-1]
    if W > WAVE:                                                      # support >= 3 over at least two chunks
        assert len(marks) >= 3 and len({c // WAVE for c in world.counted(W, 2000)}) >= 2
        assert WAVE in marks and world.counted(W, 1000 + WAVE)[0] // WAVE == 1      # only the second chunk counts
        assert world.counted(W, 1000 + W - 1)[0] // WAVE == -(-W // WAVE) - 1       # ... and only the last one
        assert len({j // WAVE for j in world.counted(W, 3000)}) == -(-W // WAVE) and not world.in_users.all()
    model = device_model(dev, world)
    items = width_items(W)
    qu, qi = np.repeat(world.queries(), items.size), np.tile(items, world.queries().size)
    for center, denominator in MODES:
        w_aff, w_support = assert_predict(model, world.ref, qu, qi, center, denominator)
        of_full = w_support[qu == full]
        assert of_full[items == 2000][0] == len(marks) and of_full[items == 777_777][0] == 0
        assert of_full[items == 3000][0] == int(world.in_users.sum())
        assert np.isnan(w_aff[qu == world.unknown]).all() and not np.isnan(w_aff[qu != world.unknown]).any()


# ---- the order witness ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def witness_world(reverse=False):
    """One row of 66 columns.  Columns 0..62: similarity 0, neighbours that rate item 7 only.  Columns 63, 64, 65:
    +2^60, -2^60, +1, neighbours that rate item 9 with 4.0.  The query user rates 2.0 and 4.0: its mean is exactly 3.
    `reverse`: the same row with its columns in descending order."""
    W = WAVE + 2
    sims = np.zeros(W, np.float32)
    sims[WAVE - 1:] = [2.0 ** 60, -(2.0 ** 60), 1.0]
    rated = [np.array([7 if j < WAVE - 1 else 9]) for j in range(W)]
    world = World(W, 77, rated, np.ones(W, bool), own=(50, 51), sims=sims)
    world.rating = np.where(world.item == 9, 4.0, np.where(world.item == 50, 2.0, np.where(world.item == 51, 4.0, 2.5)))
    if reverse:
        ids, nb, sc, ct, lengths = world.table
        world.table = frozen(ids, np.array(nb[:, ::-1]), np.array(sc[:, ::-1]), np.array(ct[:, ::-1]), lengths)
    return world.finish()


def test_sums_follow_the_column_order_across_the_wave_boundary(dev):
    """center="query", denominator="all": both sums are (2^60 - 2^60) + 1 = 1 in ascending column order, the affinity
    3 + 1 / 1 = 4.  Any association that adds column 65 to column 64 first -- one partial sum per 64-column chunk is one --
    gives 2^60 + (-2^60 + 1) = 0 in float64, a zero denominator, and so the mean 3."""
    world = witness_world()
    A = world.user_of_length(world.W)
    assert world.W == WAVE + 2 and world.ref.mean[A] == 3.0
    assert world.counted(world.W, 9) == [WAVE - 1, WAVE, WAVE + 1]   # one column of the first chunk, two of the second
    assert world.ref.affinity(A, 9, "query", "all") == (np.float32(4.0), 3)
    rev = witness_world(reverse=True)
    assert rev.ref.affinity(A, 9, "query", "all") == (np.float32(3.0), 3)     # the other order is visible in float32
    model = device_model(dev, world)
    for center, denominator in MODES:
        assert_predict(model, world.ref, [A, A, A], [9, 7, 50], center, denominator)
    aff, support = model.predict([A], [9], "query", "all")
    assert bits(aff).tolist() == bits(np.array([4.0], np.float32)).tolist() and support.tolist() == [3]
    # the same row through recommend: the same bits
    for center, denominator in MODES:
        assert_recommend(model, world.ref, [A], 5, True, 1, center, denominator)
    (ids, sc, lens), want = assert_recommend(model, world.ref, [A], 5, True, 1, "query", "all")
    assert want[0][0].tolist() == [9, 7, -1, -1, -1] and want[1][0, :2].tolist() == [4.0, 3.0] and lens.tolist() == [2]
    assert bits(sc[0, :1]).tolist() == bits(aff).tolist()


# ---- predict: more queries than the grid has waves --------------------------------------------------------------------
def test_predict_more_queries_than_waves_in_a_grid(dev):
    """2048 * 4 + 5 queries on 2048 workgroups of four waves: the first five waves take a second query -- known users, the
    two users the table lacks and user 500 (an empty row)."""
    model, ref = small_models(dev)
    users = np.append(np.unique(small_corpus()[0]), [4, 999_999])
    items = np.array([0, 7, 13, 21, 49, 900, 77])
    pu, pi = np.repeat(users, items.size), np.tile(items, users.size)
    nq = GRID_WAVES + 5
    pick = np.arange(nq) % pu.size
    tail = [int(np.flatnonzero((pu == u) & (pi == i))[0]) for u, i in ((3, 7), (4, 13), (500, 900), (999_999, 0), (10, 21))]
    pick[GRID_WAVES:] = tail
    qu, qi = pu[pick], pi[pick]
    assert nq > GRID_WAVES and qu[GRID_WAVES:].tolist() == [3, 4, 500, 999_999, 10]
    assert 3 in small_corpus()[0] and 10 in small_corpus()[0] and 4 not in users[:-2]
    for center, denominator in MODES:
        w_aff, w_support = ref.predict(pu, pi, center, denominator)           # the oracle once per unique pair
        aff, support = model.predict(qu, qi, center, denominator)
        assert np.array_equal(support.cpu().numpy(), w_support[pick])
        assert np.array_equal(bits(aff), bits(w_aff[pick]))
        assert np.isnan(w_aff[tail]).sum() == 2 and w_support.max() >= 3


# ---- recommend across table widths -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reco_world(name):
    cap = rt.max_entries()
    rng = np.random.default_rng(300 + len(name))
    if name == "one column":                  # W = 1: the one neighbour rated max_entries() items
        return World(1, 301, [np.arange(cap, dtype=np.int64) * 3], [True])
    if name in ("64", "65"):
        return width_world(int(name))
    W = MAX_WIDTH
    if name in ("two items", "above"):         # W = 1024: every neighbour rates two of 300 items
        rated = [rng.choice(300, 2, replace=False).astype(np.int64) for _j in range(W)]
        if name == "above":
            rated[5] = np.array([0, 1, 2])
        return World(W, 302, rated, np.ones(W, bool))
    assert name == "sparse"                    # W = 1024: every second column empty (j % 4 == 3) or not in users (1)
    rated = [rng.choice(300, 4, replace=False).astype(np.int64) if j % 2 == 0 else np.zeros(0, np.int64) for j in range(W)]
    return World(W, 303, rated, [j % 4 != 1 for j in range(W)])


@functools.lru_cache(maxsize=None)
def reco_model(dev_, name):
    return device_model(dev_, reco_world(name))


RECO_CASES = [(name, c, d) for name in ("one column", "64", "65", "two items", "sparse") for c, d in MODES]


@pytest.mark.parametrize("name,center,denominator", RECO_CASES)
def test_recommend_across_table_widths_at_the_cap(dev, name, center, denominator):
    """s_pu / s_start at one column, at 64 | 65 and at kUserKnnMaxWidth; the serial prefix over 1024 columns; the column
    search over runs of equal offsets (every second column gathers nothing); exactly max_entries() gathered ratings."""
    cap = rt.max_entries()
    world = reco_world(name)
    ref, W = world.ref, world.W
    full = world.user_of_length(W)
    users = world.queries()
    gathered = [ref.gathered(u) for u in users]
    assert max(gathered) <= cap and gathered[-1] == 0
    if name in ("one column", "two items", "sparse"):
        assert ref.gathered(full) == cap                              # exactly at the cap
    if name == "sparse":
        start = np.cumsum([0] + [len(world.rated[j]) if world.in_users[j] else 0 for j in range(W)])
        assert W == MAX_WIDTH and (np.diff(start)[1::2] == 0).all() and (np.diff(start)[0::2] == 4).all()
        assert not world.in_users[1] and world.in_users[3] and len(world.rated[3]) == 0
    model = reco_model(dev, name)
    assert model.gathered(users).tolist() == gathered
    row = int(np.flatnonzero(users == full)[0])
    listed = {}
    for exclude in (True, False):
        for k in (MAX_WIDTH, 7):
            (ids, sc, _lens), want = assert_recommend(model, ref, users, k, exclude, 1, center, denominator)
            listed[exclude, k] = int(want[2][row])
            if exclude:
                assert not np.isin(want[0][row], [0, 3, 6, 9]).any()  # the query users' own items
            if k == 7:
                assert listed[exclude, k] == 7
                continue
            assert listed[exclude, k] == (k if name == "one column" else listed[True, k] + 4 * (not exclude)) > 7
            live = ids >= 0                                           # every returned score is predict's, bit for bit
            qu = torch.from_numpy(users).to(dev)[:, None].expand_as(ids)[live]
            aff, support = model.predict(qu, ids[live], center, denominator)
            assert torch.equal(aff.view(torch.int32), sc[live].view(torch.int32)) and int(support.min()) >= 1


def test_one_entry_above_the_cap_at_full_width_is_refused_before_any_launch(dev, monkeypatch):
    cap = rt.max_entries()
    world = reco_world("above")
    full, users = world.user_of_length(MAX_WIDTH), world.queries()
    assert world.ref.gathered(full) == cap + 1 and world.ref.gathered(world.user_of_length(MAX_WIDTH - 1)) == cap - 1
    model = device_model(dev, world)
    assert model.gathered(users).tolist() == [world.ref.gathered(u) for u in users]
    launched = []
    monkeypatch.setattr(ops, "userknn_recommend", lambda *a, **kw: launched.append(a))
    q = int(np.flatnonzero(users == full)[0])
    with pytest.raises(ValueError, match=r"query %d \(user %d\) gathers %d ratings" % (q, full, cap + 1)):
        model.recommend(users, 10)
    assert not launched


# ---- recommend: second queries per workgroup --------------------------------------------------------------------------
@pytest.mark.parametrize("denominator", rt.DENOMINATORS)
@pytest.mark.parametrize("min_support", [1, 2])
def test_recommend_second_queries_per_workgroup(dev, denominator, min_support):
    """2048 + 3 queries on 2048 workgroups: the workgroups 0, 1, 2 take a second query of another kind than their first --
    a full list then a short one, a full list then user 500's empty row, an unknown user then a full list.  s_key, s_val,
    s_cnt and s_den are reused behind the loop-head barrier: the first query's count, its denominator or its keys beyond
    the second query's padded length must not show in the second."""
    model, ref = small_models(dev)
    uniq = np.append(np.unique(small_corpus()[0]), [4, 999_999])
    count = ref.recommend(uniq, MAX_WIDTH, True, min_support, "neighbour", denominator)[2]
    k = int(np.median(count[count > 0]))
    kinds = {"full": np.flatnonzero(count >= k), "short": np.flatnonzero((count > 0) & (count < k)),
             "empty": np.flatnonzero(uniq == 500), "unknown": np.flatnonzero(uniq >= 999_999)}
    assert k >= 3 and all(v.size >= 1 for v in kinds.values()) and kinds["full"].size > 5 < kinds["short"].size
    assert count[kinds["empty"]].tolist() == [0] and count[kinds["unknown"]].tolist() == [0]
    nq = MAX_GRID + 3
    order = ("full", "unknown", "empty", "short")
    kind = [order[q % 4] for q in range(nq)]
    kind[:3] = ["full", "full", "unknown"]
    kind[MAX_GRID:] = ["short", "empty", "full"]
    assert nq > MAX_GRID and all(kind[b] != kind[MAX_GRID + b] for b in range(3))
    pick = np.array([kinds[kd][(q // 4) % kinds[kd].size] for q, kd in enumerate(kind)])
    want = ref.recommend(uniq, k, True, min_support, "neighbour", denominator)      # the oracle once per unique user
    assert want[2][pick[0]] == want[2][pick[1]] == k > want[2][pick[MAX_GRID]] > 0 == want[2][pick[MAX_GRID + 1]]
    got = model.recommend(uniq[pick], k, True, min_support, "neighbour", denominator)
    assert np.array_equal(got[2].cpu().numpy(), want[2][pick])
    assert np.array_equal(got[0].cpu().numpy(), want[0][pick])
    assert np.array_equal(bits(got[1]), bits(want[1][pick]))

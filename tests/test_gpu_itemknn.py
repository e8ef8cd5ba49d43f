"""GPU: the item-kNN recommender (neighbours.recommend, esr_itemknn_recommend) against the CPU oracle
tests/_neighbours_ref.py, bit for bit.

The neighbour table is made on the host and wrapped as it is: 400 sparse ids, width 16 (so that a history of
max_entries / 16 ids reaches the cap exactly), rows of 0..16 partners drawn from 300 candidates -- queries share
candidates, a candidate's run spans many history positions -- and scores that are full-mantissa f32 numbers over eight
binades, so that a sum taken in another order ends in other bits (checked below, on the CPU, before anything is
compared)."""
import functools

import numpy as np
import pytest
import torch

from _neighbours_ref import ref_candidate_sums, ref_recommend
from esrecsys_amd import ops
from esrecsys_amd.wikipedia import neighbours as nbm

pytestmark = pytest.mark.gpu

WIDTH = 16
BIG = 2 ** 31 - 2


@functools.lru_cache(maxsize=None)
def host_table():
    rng = np.random.default_rng(33)
    ids = np.unique(np.concatenate([rng.integers(0, BIG, 399), [BIG]])).astype(np.int32)
    u = ids.size
    cands = np.concatenate([rng.choice(ids, 150, replace=False), rng.integers(0, BIG, 150).astype(np.int32)])
    lengths = rng.integers(0, WIDTH + 1, u).astype(np.int32)
    lengths[:4] = [0, 1, WIDTH, WIDTH]
    nb = np.full((u, WIDTH), -1, np.int32)
    sc = np.zeros((u, WIDTH), np.float32)
    for r in range(u):
        n = int(lengths[r])
        nb[r, :n] = rng.choice(cands, n, replace=False)
        sc[r, :n] = -np.sort(-(rng.random(n, dtype=np.float32) * np.float32(2.0) ** rng.integers(-7, 1, n)).astype(np.float32))
    out = (ids, nb, sc, sc.copy(), lengths)
    for x in out:
        x.setflags(write=False)
    return out


def device_table(dev, host=None):
    ids, nb, sc, ct, lengths = (torch.from_numpy(np.array(x)).to(dev) for x in (host or host_table()))
    return nbm.NeighbourTable(ids, nb, sc, ct, lengths, "both", "dice")


def queries(lengths, seed, unknown=0.1):
    """CSR histories of the given lengths: ids of the table (repeats happen and are forced), some ids it lacks."""
    rng = np.random.default_rng(seed)
    ids = host_table()[0]
    hist = []
    for n in lengths:
        h = rng.choice(ids, n).astype(np.int64)
        h[rng.random(n) < unknown] = rng.integers(0, BIG, 1)[0]
        if n >= 3:
            h[n - 1] = h[0]       # a repeat
        hist.append(h)
    off = np.concatenate([[0], np.cumsum([len(h) for h in hist])]).astype(np.int64)
    return np.concatenate(hist + [np.zeros(0, np.int64)]).astype(np.int32), off


def check(dev, history, offsets, k, exclude=True, table=None):
    host = table or host_table()
    got = nbm.recommend(device_table(dev, host), torch.from_numpy(history).to(dev), offsets, k, exclude_history=exclude)
    want = ref_recommend(host, history, offsets, k, exclude_history=exclude)
    for name, g, w in zip(("ids", "scores", "lengths"), got, want):
        w = torch.from_numpy(w)
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), name
        assert torch.equal(g.cpu(), w), name
    return want


def test_the_cap_is_a_multiple_of_the_test_width():
    assert nbm.max_entries() % WIDTH == 0 and nbm.max_entries() == ops.itemknn_max_entries()


@pytest.mark.parametrize("k", [1, 500, 1024])
@pytest.mark.parametrize("exclude", [True, False])
def test_history_lengths_up_to_the_cap(dev, exclude, k):
    """Lengths 1, 5 and the one that reaches the cap exactly, an empty query among them, repeats and unknown ids inside."""
    full = nbm.max_entries() // WIDTH
    history, offsets = queries([1, 5, 0, full, 5, 2, full, 1], seed=k)
    want = check(dev, history, offsets, k, exclude)
    assert want[2][2] == 0 and min(want[2][3], want[2][6]) > (0 if k == 1 else 100)


def test_sums_follow_the_history_order(dev):
    """Many histories that share candidates: every run of several positions is summed left to right.  The reversed
    order gives other bits for some candidate -- established here on the CPU, or the comparison would prove nothing."""
    history, offsets = queries([40] * 24 + [128] * 4, seed=7, unknown=0.0)
    host = host_table()
    differ = runs = 0
    for q in range(offsets.size - 1):
        query = history[offsets[q]:offsets[q + 1]].tolist()
        fwd, rev = ref_candidate_sums(host, query), ref_candidate_sums(host, query, reverse=True)
        differ += sum(1 for c in fwd if fwd[c] != rev[c])
        runs += len(fwd)
    assert differ >= 20, (differ, runs)
    want = check(dev, history, offsets, 1024, exclude=False)
    # and the compared sums are those: spot-check the best candidate of every query against the position-order sum
    for q in range(offsets.size - 1):
        fwd = ref_candidate_sums(host, history[offsets[q]:offsets[q + 1]].tolist())
        assert want[1][q, 0] == fwd[int(want[0][q, 0])]


def test_one_entry_above_the_cap_is_refused_before_any_launch(dev, monkeypatch):
    full = nbm.max_entries() // WIDTH
    history, offsets = queries([5, full + 1, 3], seed=3)
    launched = []
    monkeypatch.setattr(ops, "itemknn_recommend", lambda *a, **kw: launched.append(a))
    with pytest.raises(ValueError, match="query 1 has %d history ids" % (full + 1)):
        nbm.recommend(device_table(dev), torch.from_numpy(history).to(dev), offsets, 10)
    assert not launched
    with pytest.raises(ValueError, match="k = 1025"):
        nbm.recommend(device_table(dev), history, offsets, 1025)
    with pytest.raises(ValueError, match="rise from 0"):
        nbm.recommend(device_table(dev), history, offsets[:-1], 10)
    assert not launched


def test_candidates_inside_the_history_leave_nothing(dev):
    """Items 10 and 20 are each other's only neighbour; 30 points at both.  History [10, 20, 30]: every candidate is in
    it -- length 0 with exclusion, both of them without."""
    table = (np.array([10, 20, 30], np.int32), np.array([[20, -1], [10, -1], [10, 20]], np.int32),
             np.array([[0.5, 0], [0.25, 0], [0.125, 0.125]], np.float32), np.zeros((3, 2), np.float32),
             np.array([1, 1, 2], np.int32))
    history, offsets = np.array([10, 20, 30, 30], np.int32), np.array([0, 3, 4], np.int64)
    want = check(dev, history, offsets, 5, True, table)
    assert want[2].tolist() == [0, 2] and want[0][1].tolist() == [10, 20, -1, -1, -1]
    want = check(dev, history, offsets, 5, False, table)
    assert want[0][0].tolist() == [20, 10, -1, -1, -1] and want[1][0].tolist() == [0.625, 0.375, 0, 0, 0]


def test_one_query_and_none(dev):
    history, offsets = queries([5], seed=11)
    check(dev, history, offsets, 10)
    check(dev, np.zeros(0, np.int32), np.array([0, 0], np.int64), 10)           # one empty query
    ids, scores, lengths = nbm.recommend(device_table(dev), np.zeros(0, np.int32), np.array([0], np.int64), 10)
    assert tuple(ids.shape) == (0, 10) and lengths.numel() == 0                 # no query at all


def test_twice_the_same_bits_and_device_offsets(dev):
    history, offsets = queries([128, 7, 0, 33] * 8, seed=5)
    table = device_table(dev)
    a = nbm.recommend(table, torch.from_numpy(history).to(dev), torch.from_numpy(offsets).to(dev), 500)
    b = nbm.recommend(table, history, offsets, 500)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_recommend_from_a_table_the_kernel_made(dev):
    """The two parts together: a neighbour table from entries, then queries over it."""
    from _neighbours_ref import ref_neighbours
    rng = np.random.default_rng(2)
    pairs = np.unique(np.sort(rng.integers(0, 120, (3000, 2)), axis=1), axis=0)
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    count = rng.integers(1, 9, pairs.shape[0]).astype(np.float32)
    ids = np.arange(120)
    df = rng.integers(1, 30, 120).astype(np.float32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)  # noqa: E731
    table = nbm.neighbours(t(pairs[:, 0], np.int32), t(pairs[:, 1], np.int32), t(count, np.float32), t(ids, np.int32),
                           t(df, np.float32), WIDTH)
    host = ref_neighbours(pairs[:, 0], pairs[:, 1], count, ids, df, WIDTH)
    history = rng.integers(0, 130, 64).astype(np.int32)
    offsets = np.array([0, 5, 10, 30, 64], np.int64)
    got = nbm.recommend(table, history, offsets, 50)
    for g, w in zip(got, ref_recommend(host, history, offsets, 50)):
        assert torch.equal(g.cpu(), torch.from_numpy(w))

"""GPU: the user-similarity table and the user-kNN predictor (esrecsys_amd/ratings.py, esr_ratings.hip) against the CPU
oracle tests/_ratings_ref.py, bit for bit (torch.equal / array_equal on every output)."""
import functools

import numpy as np
import pytest
import torch

import _evaluate_ref as eref
from _neighbours_ref import ref_neighbours
from _ratings_ref import RefUserKnn, ref_deviations, ref_latest, ref_similarity, ref_sums
from esrecsys_amd import evaluate as ev
from esrecsys_amd import ops
from esrecsys_amd import ratings as rt
from esrecsys_amd.wikipedia import neighbours as nbm
from esrecsys_amd.wikipedia.pair_table import CooccurrenceError

pytestmark = pytest.mark.gpu

BIG = 2 ** 31 - 2
MODES = [(c, d) for c in rt.CENTERS for d in rt.DENOMINATORS]


def T():
    return ops.usersim_tile()


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- similarity ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry():
    """(user, item, dev) rows, shuffled: one item of each rater count 1, 2, T - 1, T, T + 1, 2 T + 3 -- on both sides of the
    chunk, one chunk and several, with a last chunk of one rater (T + 1) -- over a sparse pool of user ids that ends at
    2^31 - 2, deviations of both signs; and two items (ids 100, 101) whose first rater, user 3, deviates by 0 on both: the
    pairs (3, x) it makes with raters of nothing else are flat."""
    rng = np.random.default_rng(11)
    t = T()
    pool = np.unique(np.concatenate([rng.integers(1000, BIG, 3 * t), [BIG, BIG - 1, 1000]]))
    user, item, dev = [], [], []
    for it, n in enumerate([1, 2, t - 1, t, t + 1, 2 * t + 3]):
        user.append(rng.choice(pool, n, replace=False)), item.append(np.full(n, it)), dev.append(rng.integers(-5000, 5001, n))
    user[-1][0] = BIG                                                  # the largest id rates the largest item
    if BIG in user[-1][1:]:
        user[-1][1:][user[-1][1:] == BIG] = 999
    for it in (100, 101):
        user.append(np.array([3, 5, 6])), item.append(np.full(3, it)), dev.append(np.array([0, 7, -9]))
    user, item, dev = (np.concatenate(x).astype(np.int64) for x in (user, item, dev))
    p = rng.permutation(user.size)
    return frozen(user[p], item[p], dev[p])


@functools.lru_cache(maxsize=None)
def geometry_ref(min_overlap=1, min_similarity=None):
    user, item, dev = geometry()
    return ref_similarity(ref_sums(user, item, dev), min_overlap, min_similarity)


def build(dev_, rows, adds=1, **kw):
    """The builder after `adds` calls that divide the items (by item id modulo adds) among them."""
    user, item, d = rows
    b = rt.UserSimilarityBuilder(device=dev_, **kw)
    for a in range(adds):
        sel = item % adds == a
        b.add(user[sel], item[sel], d[sel])
    return b


def assert_sim(b, want, **kw):
    got = b.finalize(**kw)
    for name, g, w, dt in zip(("index", "other", "sim", "overlap"), got, want, (torch.int32, torch.int32, torch.float32,
                                                                             torch.int32)):
        assert g.dtype == dt and g.is_cuda, name
        assert np.array_equal(g.cpu().numpy(), w), name
    assert b.dropped_flat == want[4]
    return got


def test_items_on_both_sides_of_the_tile(dev):
    want = geometry_ref()
    index, other, sim, _ov = assert_sim(build(dev, geometry()), want)
    assert bool((index < other).all()) and int(other.max()) == BIG
    assert (want[2] < 0).sum() > 100 and (want[2] > 0).sum() > 100            # products of both signs: negative P too
    assert want[4] == 2                                                        # (3, 5) and (3, 6): user 3 is flat
    key = index.to(torch.int64) * (1 << 31) + other
    assert bool((key[1:] > key[:-1]).all())
    assert want[3].max() >= 2                                                  # some pairs meet in several items


def test_filters(dev):
    b = build(dev, geometry())
    assert_sim(b, geometry_ref(2), min_overlap=2)
    assert 0 < geometry_ref(2)[0].size < geometry_ref()[0].size and geometry_ref(2)[3].min() == 2
    assert_sim(b, geometry_ref(1, 0.25), min_similarity=0.25)
    assert_sim(b, geometry_ref(1, -1.0), min_similarity=-1.0)                # sim <= -1 goes: two-rater pairs of sim -1
    assert 0 < geometry_ref(1, -1.0)[0].size < geometry_ref()[0].size
    assert_sim(b, geometry_ref())                                             # the builder stays usable and unchanged


def test_one_key_under_contention(dev):
    rng = np.random.default_rng(12)
    n = 300
    user = np.tile([7, 9], n)
    item = np.repeat(np.arange(n), 2)
    d = rng.integers(-3000, 3001, 2 * n)
    want = ref_similarity(ref_sums(user, item, d))
    assert want[3].tolist() == [n]
    assert_sim(build(dev, (user, item, d)), want)


def test_launch_plan_capacity_and_division_into_adds(dev):
    rows, want = geometry(), geometry_ref()
    t = T()
    b = build(dev, rows, max_pairs_per_launch=500)                            # the 2 T + 3 item alone is above the limit
    assert b.launches >= 3 and (2 * t + 3) * (2 * t + 2) // 2 > 500
    assert_sim(b, want)
    b = build(dev, rows, capacity=2)
    assert b.rehashes > 0 and b.capacity >= 2 * want[0].size
    assert_sim(b, want)                                                       # all four planes survived the rehashes
    for adds in (2, 5):
        b = build(dev, rows, adds=adds, capacity=64, max_pairs_per_launch=3000)
        assert_sim(b, want)


def test_more_tiles_than_one_launch_grid(dev):
    """One wave per tile, 2048 workgroups of four waves at most: 8200 two-rater items are 8200 tiles."""
    rng = np.random.default_rng(13)
    n = 8200
    a = rng.integers(0, 40, n)
    user = np.stack([a, a + 1 + rng.integers(0, 40, n)], 1).reshape(-1)
    item = np.repeat(np.arange(n), 2)
    d = rng.integers(-100, 101, 2 * n)
    b = build(dev, (user, item, d))
    assert b.launches == 1 and int(rt.UserSimilarityBuilder.tiles_of(np.full(n, 2), T()).sum()) > 2048 * 4
    assert_sim(b, ref_similarity(ref_sums(user, item, d)))


@pytest.mark.parametrize("case", ["duplicate", "negative user", "negative item"])
def test_device_failures_leave_the_builder_unusable(dev, case):
    user, item, d = [1, 2, 3, 2], [4, 4, 4, 4], [1, 2, 3, 4]                  # user 2 rates item 4 twice
    match = "bits 128"
    if case == "negative user":
        user, match = [1, 2, -3, 5], "bits 2"
    if case == "negative item":
        item, match = [-4, -4, -4, -4], "bits 2"
        user = [1, 2, 3, 5]
    b = rt.UserSimilarityBuilder(capacity=16, device=dev)
    with pytest.raises(CooccurrenceError, match=match):
        b.add(user, item, d)
    with pytest.raises(CooccurrenceError, match="unusable"):
        b.add([1, 2], [9, 9], [1, 1])
    with pytest.raises(CooccurrenceError, match="unusable"):
        b.finalize()
    assert_sim(build(dev, (np.array([1, 2]), np.array([9, 9]), np.array([1, 1]))),      # and a fresh builder is sound
               ref_similarity(ref_sums([1, 2], [9, 9], [1, 1])))


# ---- through neighbours -------------------------------------------------------------------------------------------------
def to_dev(dev_, a, dt):
    return torch.from_numpy(np.array(a, dt)).to(dev_)                   # (a copy: the cached arrays are read-only)


def table_of(dev_, index, other, sim, users, k):
    return nbm.neighbours(to_dev(dev_, index, np.int32), to_dev(dev_, other, np.int32), to_dev(dev_, sim, np.float32),
                          to_dev(dev_, users, np.int32), None, k, "both", "count")


def assert_table(table, want):
    for name, w in zip(("ids", "neighbours", "scores", "counts", "lengths"), want):
        assert np.array_equal(getattr(table, name).cpu().numpy(), w), name


@pytest.mark.parametrize("k", [1, 5, 64, 1024])
def test_negative_similarities_through_neighbours(dev, k):
    """score="count" ranks by the similarity itself: its order key must be total over signed floats."""
    index, other, sim, _ov, _flat = geometry_ref()
    users = np.unique(np.concatenate([index, other, [0, 3]]))                  # two users without entries
    want = ref_neighbours(index, other, sim, users, None, k, "both", "count")
    assert_table(table_of(dev, index, other, sim, users, k), want)
    assert (want[2] < 0).any() and (want[2] > 0).any() and want[4].min() == 0


def test_similarity_ties_go_to_the_lower_id(dev):
    index = [1, 1, 1, 1, 1, 2, 4]
    other = [9, 4, 7, 2, 5, 9, 9]
    sim = [0.5, -0.25, 0.5, -0.25, 0.5, -0.25, -0.25]
    users = [1, 2, 4, 5, 7, 9]
    want = ref_neighbours(index, other, sim, users, None, 4, "both", "count")
    assert want[1][0].tolist() == [5, 7, 9, 2] and want[1][5].tolist() == [1, 2, 4, -1]
    assert_table(table_of(dev, index, other, sim, users, 4), want)


# ---- predictor ----------------------------------------------------------------------------------------------------------
def pipeline(dev_, user, item, rating, k, min_overlap=2, frac_bits=12):
    """(model, oracle) of the whole chain from one rating per pair."""
    users, mean, d = rt.rating_deviations(to_dev(dev_, user, np.int32), to_dev(dev_, rating, np.float64), frac_bits)
    b = rt.UserSimilarityBuilder(capacity=1 << 10, device=dev_).add(user, item, d)
    index, other, sim, _ov = b.finalize(min_overlap=min_overlap)
    table = nbm.neighbours(index, other, sim, users, None, k, "both", "count")
    model = rt.UserKnn(table, user, item, rating, users, mean)
    r_users, r_mean, r_dev = ref_deviations(user, rating, frac_bits)
    assert users.tolist() == r_users and mean.tolist() == [float(x) for x in r_mean] and d.tolist() == r_dev
    r_index, r_other, r_sim, _o, _f = ref_similarity(ref_sums(user, item, r_dev), min_overlap)
    r_table = ref_neighbours(r_index, r_other, r_sim, np.array(r_users), None, k, "both", "count")
    assert_table(table, r_table)
    return model, RefUserKnn(r_table, user, item, rating, r_users, r_mean)


@functools.lru_cache(maxsize=None)
def small_corpus():
    """60 users x 50 items, 30 % rated in half stars; user 500 rates only item 900 (alone: an empty table row)."""
    rng = np.random.default_rng(17)
    user, item = np.nonzero(rng.random((60, 50)) < 0.3)
    rating = rng.integers(1, 11, user.size) / 2.0
    return frozen(np.append(user * 7 + 3, 500), np.append(item, 900), np.append(rating, 2.5))


@functools.lru_cache(maxsize=None)
def small_models(dev_):
    return pipeline(dev_, *small_corpus(), k=5)


@pytest.mark.parametrize("center,denominator", MODES)
def test_predict_every_user_and_item(dev, center, denominator):
    model, ref = small_models(dev)
    users = np.append(np.unique(small_corpus()[0]), [4, 999_999])             # two users the table lacks
    items = np.append(np.arange(50), [900, 77])                               # an item one user rated, one nobody rated
    qu, qi = np.repeat(users, items.size), np.tile(items, users.size)
    aff, support = model.predict(qu, qi, center, denominator)
    w_aff, w_support = ref.predict(qu, qi, center, denominator)
    assert aff.dtype == torch.float32 and support.dtype == torch.int32
    assert np.array_equal(support.cpu().numpy(), w_support)
    assert np.array_equal(aff.cpu().numpy().view(np.uint32), w_aff.view(np.uint32))
    absent = np.isin(qu, [4, 999_999])
    assert np.isnan(w_aff[absent]).all() and (w_support[absent] == 0).all() and not np.isnan(w_aff[~absent]).any()
    assert 0 < (w_support == 0).sum() and w_support.max() >= 3                # nobody / several neighbours rated it
    lone = qu == 500
    assert (w_support[lone] == 0).all() and (w_aff[lone] == np.float32(2.5)).all()        # an empty row: the mean


@pytest.mark.parametrize("center,denominator", MODES)
@pytest.mark.parametrize("exclude_rated,min_support,k", [(True, 1, 10), (False, 2, 1024), (True, 0, 3), (False, 6, 5)])
def test_recommend_against_the_oracle_and_predict(dev, center, denominator, exclude_rated, min_support, k):
    model, ref = small_models(dev)
    users = np.append(np.unique(small_corpus()[0]), [4, 999_999])
    ids, sc, lens = model.recommend(users, k, exclude_rated, min_support, center, denominator)
    w_ids, w_sc, w_lens = ref.recommend(users, k, exclude_rated, min_support, center, denominator)
    assert tuple(ids.shape) == (users.size, k) and ids.dtype == torch.int32 and lens.dtype == torch.int32
    assert np.array_equal(lens.cpu().numpy(), w_lens)
    assert np.array_equal(ids.cpu().numpy(), w_ids)
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), w_sc.view(np.uint32))
    if min_support == 6:
        assert not w_lens.any()                                               # five neighbours: support 6 never happens
        return
    assert w_lens[-3:].tolist() == [0, 0, 0] and (w_lens[:-3] >= 1).mean() > 0.9
    assert k != 1024 or (w_lens < k).all()                                    # k above every candidate count
    # every returned (user, item): the score is predict's, bit for bit
    live = ids >= 0
    qu = torch.from_numpy(users).to(dev)[:, None].expand_as(ids)[live]
    aff, support = model.predict(qu, ids[live], center, denominator)
    assert torch.equal(aff.view(torch.int32), sc[live].view(torch.int32))
    assert int(support.min()) >= max(min_support, 1)             # a candidate is an item some neighbour rated


def handmade(dev_, index, other, sim, user, item, rating, k):
    users, mean, _d = rt.rating_deviations(to_dev(dev_, user, np.int32), to_dev(dev_, rating, np.float64))
    table = table_of(dev_, index, other, sim, users.cpu().numpy(), k)
    r_users, r_mean, _rd = ref_deviations(user, rating)
    r_table = ref_neighbours(index, other, np.asarray(sim, np.float32), np.array(r_users), None, k, "both", "count")
    return rt.UserKnn(table, user, item, rating, users, mean), RefUserKnn(r_table, user, item, rating, r_users, r_mean)


def test_cancelling_similarities_and_affinity_ties(dev):
    """User 1 has the neighbours 2 (+0.5) and 3 (-0.5): under denominator="all" the row sums to 0 and the affinity is the
    user's mean.  User 2 rates the items 9, 3, 5 alike and 3 rates none of them: equal affinities, ascending item id."""
    user = [1, 1, 2, 2, 2, 2, 3, 3]
    item = [1, 2, 9, 3, 5, 1, 1, 2]
    rating = [4.0, 2.0, 4.5, 4.5, 4.5, 1.0, 3.0, 5.0]
    model, ref = handmade(dev, [1, 1], [2, 3], [0.5, -0.5], user, item, rating, 5)
    for center, denominator in MODES:
        got = model.recommend([1, 2, 3], 6, True, 1, center, denominator)
        want = ref.recommend([1, 2, 3], 6, True, 1, center, denominator)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w)
        assert want[0][0].tolist() == [3, 5, 9, -1, -1, -1]
        aff, support = model.predict([1, 1, 1], [1, 9, 2], center, denominator)
        w_aff, w_support = ref.predict([1, 1, 1], [1, 9, 2], center, denominator)
        assert np.array_equal(aff.cpu().numpy(), w_aff) and support.tolist() == w_support.tolist() == [2, 1, 1]
        if denominator == "all":
            assert w_aff.tolist() == [3.0, 3.0, 3.0] and want[1][0, :3].tolist() == [3.0, 3.0, 3.0]   # den == 0: the mean
        else:
            assert len(set(want[1][0, :3].tolist())) == 1 and want[1][0, 0] != np.float32(3.0)


def test_a_query_at_the_cap_and_one_entry_above_it(dev):
    """User 1's neighbours 10 and 11 rated max_entries() items between them; user 2 has them and 12, who rated one."""
    cap = rt.max_entries()
    rng = np.random.default_rng(19)
    half = cap // 2
    items10, items11 = np.arange(half) * 2, np.arange(half) * 3 + 1              # they overlap on a sixth of the items
    user = np.concatenate([[1, 2], np.full(half, 10), np.full(half, 11), [12]])
    item = np.concatenate([[5000, 5000], items10, items11, [7]])
    rating = np.concatenate([[3.0, 4.0], rng.integers(1, 11, cap) / 2.0, [1.5]])
    model, ref = handmade(dev, [1, 1, 2, 2, 2], [10, 11, 10, 11, 12], [0.9, -0.4, 0.3, 0.6, 0.2], user, item, rating, 3)
    assert ref.gathered(1) == cap and ref.gathered(2) == cap + 1
    assert model.gathered([1, 2, 10, 77]).tolist() == [cap, cap + 1, 2, 0]
    for center, denominator in MODES:
        got = model.recommend([1, 12], 1024, True, 1, center, denominator)
        want = ref.recommend([1, 12], 1024, True, 1, center, denominator)
        assert want[2][0] == 1024
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w)
    with pytest.raises(ValueError, match=r"query 1 \(user 2\) gathers %d ratings" % (cap + 1)):
        model.recommend([1, 2], 10)


def test_user_knn_argument_checks(dev):
    model, _ref = small_models(dev)
    user, item, rating = small_corpus()
    with pytest.raises(ValueError, match="rated twice"):
        rt.UserKnn(model.table, np.append(user, user[0]), np.append(item, item[0]), np.append(rating, 1.0),
                   model.users, model.mean)
    with pytest.raises(ValueError, match="not in users"):
        rt.UserKnn(model.table, np.append(user, 1), np.append(item, 1), np.append(rating, 1.0), model.users, model.mean)
    with pytest.raises(ValueError, match="one length"):
        rt.UserKnn(model.table, user, item, rating, model.users, model.mean[:-1])
    empty = model.recommend(np.zeros(0, np.int32), 5)
    assert tuple(empty[0].shape) == (0, 5) and model.predict([], [])[0].numel() == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_ratings_to_ranking_metrics_end_to_end(dev):
    """200 users, 80 Zipf-popular items, every pair rated up to three times; the latest rating counts.  Per user the items
    whose latest rating is 4 or better and whose id is 0 mod 3 are held out as the truth; the rest trains."""
    rng = np.random.default_rng(23)
    n = 6000
    user = rng.integers(0, 200, n) * 11 + 5
    item = (rng.zipf(1.3, n) - 1) % 80
    rating = rng.integers(1, 11, n) / 2.0
    tstamp = rng.integers(0, 1000, n)
    u, i, r = rt.latest_ratings(to_dev(dev, user, np.int32), to_dev(dev, item, np.int32), to_dev(dev, rating, np.float64),
                                to_dev(dev, tstamp, np.int64))
    wu, wi, wr = (np.array(x) for x in ref_latest(user, item, rating, tstamp))
    assert u.tolist() == wu.tolist() and i.tolist() == wi.tolist() and r.tolist() == wr.tolist()
    held = (wr >= 4.0) & (wi % 3 == 0)
    tu, ti, tr = wu[~held], wi[~held], wr[~held]
    model, ref = pipeline(dev, tu, ti, tr, k=5)
    queries = np.unique(wu)
    truth = [wi[held & (wu == q)] for q in queries]
    t_off = np.concatenate([[0], np.cumsum([t.size for t in truth])])
    truth = np.concatenate(truth).astype(np.int32)
    rec_ids, rec_sc, rec_len = model.recommend(queries, 20)
    w_ids, w_sc, w_len = ref.recommend(queries, 20)
    assert np.array_equal(rec_ids.cpu().numpy(), w_ids) and np.array_equal(rec_len.cpu().numpy(), w_len)
    assert np.array_equal(rec_sc.cpu().numpy().view(np.uint32), w_sc.view(np.uint32))
    got = ev.ranking_metrics(rec_ids, rec_len, truth, t_off, ks=(5, 20))
    want = eref.ranking_metrics(w_ids, w_len, truth, t_off, (5, 20))
    for name in ("hits", "first_hit", "valid", "precision", "recall", "rr", "ap", "ndcg"):
        assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), name
    assert int(want["hits"][:, 1].sum()) > 50 and int(want["valid"].sum()) > 150

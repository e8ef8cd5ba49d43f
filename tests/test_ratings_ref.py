"""CPU: the oracle tests/_ratings_ref.py pinned on a hand-worked example, the torch plumbing of esrecsys_amd/ratings.py
(``latest_ratings``, ``rating_deviations``: they run where their inputs live) against it, the fixed-point similarity
against a direct float64 Pearson within the quantisation's own bound, and every refusal that needs no device."""
import math
import types

import numpy as np
import pytest
import torch

from _neighbours_ref import ref_neighbours
from _ratings_ref import RefUserKnn, ref_deviations, ref_latest, ref_sim, ref_similarity, ref_sums, vec_similarity
from esrecsys_amd import ratings as rt

# 3 users x 4 items.  Means: user 1 -> 4, user 2 -> 3.5, user 3 -> 3.
USER = [1, 1, 1, 2, 2, 2, 2, 3, 3, 3]
ITEM = [10, 20, 30, 10, 20, 30, 40, 10, 20, 40]
RATING = [5.0, 3.0, 4.0, 4.0, 2.0, 3.0, 5.0, 2.0, 4.0, 3.0]


def test_oracle_on_the_hand_worked_example():
    users, mean, dev = ref_deviations(USER, RATING, frac_bits=1)
    assert users == [1, 2, 3] and mean == [4.0, 3.5, 3.0]
    assert dev == [2, -2, 0, 1, -3, -1, 3, -2, 2, 0]                 # twice the deviations
    sums = ref_sums(USER, ITEM, dev)
    assert sums == {(1, 2): [3, 2 * 1 + 2 * 3 + 0, 4 + 4 + 0, 1 + 9 + 1],          # items 10, 20, 30
                    (1, 3): [2, -4 - 4, 8, 8],                                     # items 10, 20
                    (2, 3): [3, -2 - 6 + 0, 1 + 9 + 9, 4 + 4 + 0]}                 # items 10, 20, 40
    index, other, sim, overlap, flat = ref_similarity(sums)
    assert index.tolist() == [1, 1, 2] and other.tolist() == [2, 3, 3] and overlap.tolist() == [3, 2, 3] and flat == 0
    want = [8 / math.sqrt(8 * 11), -1.0, -8 / math.sqrt(19 * 8)]
    assert np.allclose(sim, want, rtol=0, atol=1e-7) and sim[1] == np.float32(-1.0)
    assert ref_similarity(sums, min_overlap=3)[0].tolist() == [1, 2]
    assert ref_similarity(sums, min_similarity=-0.7)[1].tolist() == [2, 3]        # -1 <= -0.7 is dropped
    assert ref_similarity(sums, min_similarity=-1.0)[1].tolist() == [2, 3]        # sim <= min_similarity: -1 goes too

    table = ref_neighbours(index, other, sim, np.array(users), None, 2, "both", "count")
    assert table[1].tolist() == [[2, 3], [1, 3], [2, 1]]             # descending similarity, negative ones behind
    model = RefUserKnn(table, USER, ITEM, RATING, users, mean)
    s12, s13 = float(sim[0]), float(sim[1])
    # user 1, item 40: neighbour 2 rated it 5 (mean 3.5), neighbour 3 rated it 3 (mean 3)
    aff, support = model.affinity(1, 40)                             # Resnick: centred on the neighbours, sum |s|
    assert support == 2 and aff == np.float32(4 + (s12 * 1.5 + s13 * 0.0) / (s12 + 1.0))
    aff, support = model.affinity(1, 40, "query", "all")             # as printed: centred on user 1, sum s over the row
    assert support == 2 and aff == np.float32(4 + (s12 * 1.0 + s13 * -1.0) / (s12 + s13))
    aff, support = model.affinity(1, 40, "query", "rated")
    assert aff == np.float32(4 + (s12 * 1.0 + s13 * -1.0) / (s12 + 1.0))
    aff, support = model.affinity(1, 40, "neighbour", "all")
    assert aff == np.float32(4 + (s12 * 1.5) / (s12 + s13))
    assert model.affinity(1, 99) == (np.float32(4.0), 0)             # nobody rated it: the user's mean
    a, s = model.affinity(7, 10)
    assert np.isnan(a) and s == 0                                    # a user the table lacks
    ids, sc, lens = model.recommend([1, 3, 7], 3)
    assert ids.tolist() == [[40, -1, -1], [30, -1, -1], [-1, -1, -1]] and lens.tolist() == [1, 1, 0]
    assert sc[0, 0] == model.affinity(1, 40)[0]
    ids, _sc, lens = model.recommend([1], 4, exclude_rated=False)
    assert sorted(ids[0].tolist()) == [10, 20, 30, 40] and lens.tolist() == [4]
    assert model.recommend([1], 4, exclude_rated=False, min_support=2)[0][0].tolist().count(-1) == 1   # 30: one rater
    assert model.gathered(1) == 4 + 3 and model.gathered(7) == 0


def test_a_flat_user_is_dropped_and_counted():
    sums = ref_sums([1, 1, 2, 2], [10, 20, 10, 20], [0, 0, 3, -3])
    assert sums == {(1, 2): [2, 0, 0, 18]}
    assert ref_similarity(sums)[4] == 1 and ref_similarity(sums)[0].size == 0


def test_the_vectorised_similarity_equals_the_loop_version():
    """``vec_similarity`` (the oracle of test_gpu_ratings_scale.py) against ``ref_similarity(ref_sums(...))`` on the
    rows of test_gpu_ratings.geometry(): every array equal, the float32 similarities through their bits, under every
    filter that the GPU tests use; and on the inputs that end in no pair at all."""
    from test_gpu_ratings import geometry          # host arrays; the tile size comes from the library, no device
    user, item, dev = geometry()
    kept = set()
    for min_overlap, min_similarity in ((1, None), (2, None), (1, 0.0), (1, 0.25), (1, -1.0), (2, 0.0), (3, None)):
        want = ref_similarity(ref_sums(user, item, dev), min_overlap, min_similarity)
        got = vec_similarity(user, item, dev, min_overlap, min_similarity)
        for g, w in zip(got[:4], want[:4]):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
        assert got[4] == want[4] == 2 and isinstance(got[4], int)
        kept.add(want[0].size)
    assert len(kept) >= 5 and min(kept) < max(kept) // 2             # the filters cut differently, and deep
    for rows in (([], [], []), ([1, 2], [7, 8], [3, 4]), ([1, 2], [7, 7], [0, 5])):        # nothing, no pair, one flat pair
        got, want = vec_similarity(*rows), ref_similarity(ref_sums(*rows))
        assert all(g.dtype == w.dtype and g.size == w.size == 0 for g, w in zip(got[:4], want[:4])) and got[4] == want[4]
    with pytest.raises(AssertionError, match="occurs twice"):
        vec_similarity([1, 1], [7, 7], [3, 4])


def test_latest_ratings_against_the_oracle():
    rng = np.random.default_rng(3)
    n = 400
    user, item = rng.integers(0, 12, n), rng.integers(0, 9, n)
    rating = rng.integers(1, 11, n) / 2.0
    tstamp = rng.integers(0, 40, n)                                  # many ties: the later row wins
    u, i, r = rt.latest_ratings(user, item, rating, tstamp)
    wu, wi, wr = ref_latest(user, item, rating, tstamp)
    assert u.dtype == torch.int32 and i.dtype == torch.int32
    assert u.tolist() == wu and i.tolist() == wi and r.tolist() == wr
    assert len(wu) == len(set(zip(user.tolist(), item.tolist())))
    u2, i2, r2 = rt.latest_ratings(torch.tensor([5, 5]), torch.tensor([1, 1]), torch.tensor([2.0, 3.0]), torch.tensor([9, 9]))
    assert (u2.tolist(), i2.tolist(), r2.tolist()) == ([5], [1], [3.0])
    with pytest.raises(ValueError, match="one length"):
        rt.latest_ratings([1, 2], [1], [1.0, 2.0], [0, 0])


def test_rating_deviations_against_the_oracle():
    rng = np.random.default_rng(4)
    n = 500
    user = rng.integers(0, 30, n) * 71_582_788                       # sparse ids up to 2 075 900 852
    rating = rng.integers(1, 11, n) / 2.0                            # half stars: every partial sum is exact
    for frac_bits in (0, 1, 12, 20):
        users, mean, dev = rt.rating_deviations(user, rating, frac_bits)
        wu, wm, wd = ref_deviations(user, rating, frac_bits)
        assert users.dtype == torch.int32 and mean.dtype == torch.float64 and dev.dtype == torch.int32
        assert users.tolist() == wu and mean.tolist() == [float(m) for m in wm] and dev.tolist() == wd
    users, mean, dev = rt.rating_deviations([1, 1, 1, 1], [0.5, 1.5, 1.0, 1.0], 0)      # deviations -0.5, 0.5: half to even
    assert dev.tolist() == [0, 0, 0, 0]
    users, mean, dev = rt.rating_deviations([1, 1, 1, 1], [0.0, 3.0, 1.5, 1.5], 0)      # -1.5, 1.5 -> -2, 2
    assert dev.tolist() == [-2, 2, 0, 0]
    with pytest.raises(ValueError, match="frac_bits"):
        rt.rating_deviations([1], [1.0], 31)
    with pytest.raises(ValueError, match="one length"):
        rt.rating_deviations([1, 2], [1.0])


def test_fixed_point_similarity_is_within_the_quantisation_bound_of_a_float64_pearson():
    """frac_bits = 12.  In rating units a stored deviation is e = d + delta with |delta| <= h = 2^-13 (half a grid step;
    the scaling by 2^12 is exact).  With |d| <= m and n co-rated items every one of the three sums moves by at most
    eps = n (2 m h + h^2).  With ra = eps / Qa, rb = eps / Qb (both < 1) and g = 1 / sqrt((1 - ra) (1 - rb)):
        |sim' - sim| <= eps g / sqrt(Qa Qb)  +  |sim| (g - 1)  <=  eps g / sqrt(Qa Qb) + (g - 1)
    plus the final rounding to float32 (2^-24 for |sim| <= 1) and 1e-12 for the float64 evaluations on both sides.  A pair
    with ra >= 1 or rb >= 1 is not constrained by the quantisation and is left out; the data leave few of those."""
    rng = np.random.default_rng(8)
    frac_bits, h = 12, 2.0 ** -13
    n_users, n_items = 25, 40
    user, item = np.nonzero(rng.random((n_users, n_items)) < 0.45)
    rating = rng.integers(1, 11, user.size) / 2.0
    users, mean, dev = ref_deviations(user, rating, frac_bits)
    mean_of = dict(zip(users, mean))
    d = {(int(u), int(i)): float(np.float64(r) - mean_of[int(u)]) for u, i, r in zip(user, item, rating)}
    m = max(abs(x) for x in d.values())
    sums = ref_sums(user, item, dev)
    bounds = []
    for (a, b), (n, P, Qa, Qb) in sums.items():
        common = [i for i in range(n_items) if (a, i) in d and (b, i) in d]
        assert len(common) == n
        x, y = np.array([d[(a, i)] for i in common]), np.array([d[(b, i)] for i in common])
        qa, qb = float(np.dot(x, x)), float(np.dot(y, y))
        eps = n * (2 * m * h + h * h)
        if qa <= eps or qb <= eps or Qa == 0 or Qb == 0:
            continue
        g = 1.0 / math.sqrt((1 - eps / qa) * (1 - eps / qb))
        bound = eps * g / math.sqrt(qa * qb) + (g - 1) + 2.0 ** -24 + 1e-12
        direct = float(np.dot(x, y)) / math.sqrt(qa * qb)
        assert abs(float(ref_sim(P, Qa, Qb)) - direct) <= bound, (a, b, n)
        bounds.append(bound)
    assert len(bounds) >= 0.9 * len(sums) and len(bounds) > 200
    assert float(np.median(bounds)) < 1e-2                           # the bound is not vacuous on this data


# ---- refusals that need no device -------------------------------------------------------------------------------------
def builder(**kw):
    return rt.UserSimilarityBuilder(device="cuda:0", **kw)          # a device NAME: nothing is touched before a launch


def test_exactness_bound_names_frac_bits():
    b = builder()
    with pytest.raises(ValueError, match="frac_bits"):
        b.add([1, 2], [7, 7], [1 << 27, 1])                          # (2^27)^2 x 1 item = 2^54
    b.add([1], [7], [(1 << 26) - 1])                                 # one item below the bound (and nothing to launch)
    with pytest.raises(ValueError, match="2\\^53"):
        b.add([1, 1, 1], [8, 9, 10], [1, 1, 1])                      # the item count is part of it: (2^26 - 1)^2 x 4
    b2 = builder()
    b2.add([1], [7], [1 << 25])
    b2.add([1, 1], [8, 9], [1, 1])                                   # 2^50 x 3 < 2^53
    with pytest.raises(ValueError, match="frac_bits"):
        b2.add(np.arange(6), np.arange(100, 106), np.ones(6, np.int64))      # 2^50 x 9 >= 2^53


def test_an_item_repeated_across_adds_is_refused():
    b = builder()
    b.add([1, 2], [10, 20], [5, -5])                                 # single-rater items: no pair, no launch, no device
    with pytest.raises(ValueError, match="item 20 was given in an earlier add"):
        b.add([3, 4], [30, 20], [1, 1])
    b.add([3], [30], [1])                                            # the refused add left nothing behind
    assert b.launches == 0


def test_add_and_finalize_argument_checks():
    b = builder()
    with pytest.raises(ValueError, match="one length"):
        b.add([1, 2], [1], [1, 1])
    with pytest.raises(TypeError, match="integer"):
        b.add([1, 2], [1, 1], [0.5, 1.0])
    with pytest.raises(ValueError, match="min_overlap"):
        b.finalize(min_overlap=0)
    with pytest.raises(ValueError, match="NaN"):
        b.finalize(min_similarity=float("nan"))
    assert rt.UserSimilarityBuilder.tiles_of(np.array([0, 1, 2, 64, 65, 131]), 64).tolist() == [0, 0, 1, 1, 3, 6]


def cpu_table():
    z = torch.zeros((2, 3), dtype=torch.int32)
    return types.SimpleNamespace(ids=torch.tensor([1, 2], dtype=torch.int32), neighbours=z, scores=z.float(),
                                 counts=z.float(), lengths=torch.zeros(2, dtype=torch.int32), k=3)


def test_cpu_tensors_are_refused():
    with pytest.raises(TypeError, match="no CPU fallback"):
        rt.UserKnn(cpu_table(), [1], [1], [1.0], [1], [1.0])


def test_modes_and_k_are_checked_before_anything_else():
    model = rt.UserKnn.__new__(rt.UserKnn)                           # no table, no device: the checks come first
    for call in (lambda **kw: model.predict([1], [1], **kw), lambda **kw: model.recommend([1], 5, **kw)):
        with pytest.raises(ValueError, match="center"):
            call(center="item")
        with pytest.raises(ValueError, match="denominator"):
            call(denominator="some")
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="k = "):
            model.recommend([1], k)
    with pytest.raises(ValueError, match="min_support"):
        model.recommend([1], 5, min_support=-1)
    with pytest.raises(ValueError, match="one length"):
        model.predict([1, 2], [1])

"""GPU: esr_rerank.hip against the restatement of tests/_rerank_ref.py -- bit for bit on exact tables across ranks, widths,
n_out, lengths and both launch forms (rows staged in LDS or read from global memory), independence of the batch, of n_out and
of the grid, the project's bound on random tables (per round, recomputed in fp64 from the kernel's own picks), the failure
bits, and ``diversify`` on a planted model.

Measured on an MI355X (profiles/rerank/parity_errors.json): see DESIGN.md section 4m."""
import json
import os

import numpy as np
import pytest

import _rerank_ref as rref

pytestmark = pytest.mark.gpu

DS = (4, 8, 32, 64, 100, 128)
WIDTHS = (1, 2, 63, 64, 65, 257, 1024)
LAMS = (0.0, 0.25, 0.5, 0.75, 1.0)
KS = (1, 2, 10, 64, 100, 1000, 5000)
NI = 300
MEASURED = {}


def _t(a, dt=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mmr(rows, cand, rel, lengths, lam, n_out, want_failed=0):
    """ops.rerank_mmr on host arrays: (pos, item, rel, value, length) as arrays; the failure word is checked"""
    import torch
    from esrecsys_amd import ops
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = ops.rerank_mmr(_t(rows, np.float32), _t(cand, np.int32), _t(rel, np.float32), _t(lengths, np.int32), lam, n_out,
                         failed=word)
    assert int(word.item()) == want_failed
    return tuple(o.cpu().numpy() for o in out)


def _ils(rows, cand, lengths, ks, want_failed=0):
    import torch
    from esrecsys_amd import ops
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    ils, valid = ops.rerank_ils(_t(rows, np.float32), _t(cand, np.int32), _t(lengths, np.int32), ks, failed=word)
    assert int(word.item()) == want_failed
    return ils.cpu().numpy(), valid.cpu().numpy()


def _same_mmr(got, want, n=None):
    """the five outputs bit for bit; `want` = (pos, item, rel, value fp64 or f32, length) cut to its first n rounds"""
    pos, item, rel, value, length = want
    n = pos.shape[1] if n is None else n
    assert rref.is_f32(value)
    assert np.array_equal(got[0], pos[:, :n]) and np.array_equal(got[1], item[:, :n])
    assert np.array_equal(_bits(got[2]), _bits(rel[:, :n])) and np.array_equal(_bits(got[3]), _bits(value[:, :n]))
    assert np.array_equal(got[4], np.minimum(length, n))


def _exact_case(D, width, nq, seed, dup=True):
    rng = np.random.default_rng(seed)
    rows = rref.exact_table(rng, NI, D)
    cand = rng.integers(0, NI, (nq, width)).astype(np.int32)
    rel = rref.exact_rel(rng, (nq, width))
    if dup and width >= 63:
        cand[:, 7], cand[:, 40] = cand[:, 3], cand[:, 3]                    # an item three times in every list
        rel[0, :] = 0.5                                                      # an all-equal rel row
    return rows, cand, rel


def _exact_ref(rows, cand, rel, lengths, lam):
    grams = [rref.gram_of(rows, c) for c in cand]
    assert all(rref.is_f32(g) for g in grams)
    return rref.mmr_ref(rows, cand, rel, lengths, lam, cand.shape[1], np.float64, grams)


# ---- bit for bit on exact tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_exact_tables_bit_for_bit(D):
    from esrecsys_amd import ops
    forms = set()
    for width in WIDTHS:
        rows, cand, rel = _exact_case(D, width, 5, 1000 * D + width)
        lengths = np.array([width, 0, 1, (width + 1) // 2, width + 7], np.int32)
        forms.add(ops.rerank_geometry(D, width)["staged"])
        grams = [rref.gram_of(rows, c) for c in cand]
        for lam in LAMS:
            want = rref.mmr_ref(rows, cand, rel, lengths, lam, width, np.float64, grams)
            assert want[5] == 0 and want[4].tolist() == [width, 0, min(1, width), (width + 1) // 2, width]
            for n_out in sorted({1, min(2, width), width}):
                _same_mmr(_mmr(rows, cand, rel, lengths, lam, n_out), want[:5], n_out)
            full = [0, 4]                                                    # without lengths: the two full rows
            _same_mmr(_mmr(rows, cand[full], rel[full], None, lam, width), tuple(w[full] for w in want[:5]))
        wi, wv, wf = rref.ils_ref(rows, cand, lengths, KS, np.float64, grams)
        gi, gv = _ils(rows, cand, lengths, KS)
        assert np.array_equal(_bits(gi), _bits(wi)) and np.array_equal(gv, wv) and wf == 0
        gi, gv = _ils(rows, cand[full], None, KS)
        assert np.array_equal(_bits(gi), _bits(wi[full])) and np.array_equal(gv, wv[full])
    assert forms == ({0, 1} if D * 1024 * 4 > rref.STAGE_BYTES else {1})


def test_exact_tables_are_exact_in_the_restatement():
    """what the test above leans on, shown and not assumed: at the largest shape every sim, every product and every v of
    every round is a float32 number, and the similarities handed in as a matrix product equal the rule's chain"""
    rows, cand, rel = _exact_case(128, 1024, 1, 7)
    gram = rref.gram_of(rows, cand[0])
    assert rref.is_f32(gram) and np.abs(gram).max() <= 512
    assert np.array_equal(gram[5], rref.sim_rows(rows[cand[0]], rows[cand[0, 5]], np.float32).astype(np.float64))
    for lam in LAMS:
        r = rref.mmr_query(rows, cand[0], rel[0], 1024, lam, 1024, np.float64, gram=gram)
        oml = np.float64(np.float32(1.0) - np.float32(lam))
        assert rref.is_f32(oml * gram) and rref.is_f32(np.float64(np.float32(lam)) * rel[0].astype(np.float64))
        assert all(rref.is_f32(v[np.isfinite(v)]) for v in r["values"]) and r["length"] == 1024


@pytest.mark.parametrize("D,below", [(64, 512), (128, 256)])
def test_both_sides_of_the_staging_budget(D, below):
    """the widths just below and just above the budget really run the two forms, each equals the restatement, and one
    list gives the same bits through both (random rows: the equality is of the expression, not of exact inputs)"""
    from esrecsys_amd import ops
    g0, g1 = ops.rerank_geometry(D, below), ops.rerank_geometry(D, below + 1)
    assert g0["staged"] == 1 and g1["staged"] == 0 and below * D * 4 == g0["stage_bytes"]
    assert g0["lds_bytes"] == 16 * below + g0["stage_bytes"] and g1["lds_bytes"] == 16 * (below + 1)
    for width in (below, below + 1):
        rows, cand, rel = _exact_case(D, width, 2, D + width)
        lengths = np.array([width, width - 3], np.int32)
        for lam in (0.5, 0.75):
            _same_mmr(_mmr(rows, cand, rel, lengths, lam, width), _exact_ref(rows, cand, rel, lengths, lam)[:5])
        wi, wv, _ = rref.ils_ref(rows, cand, lengths, KS, np.float64, [rref.gram_of(rows, c) for c in cand])
        gi, gv = _ils(rows, cand, lengths, KS)
        assert np.array_equal(_bits(gi), _bits(wi)) and np.array_equal(gv, wv)
    rng = np.random.default_rng(D)
    rows = rng.standard_normal((NI, D)).astype(np.float32)
    cand, rel = rng.integers(0, NI, (3, below)).astype(np.int32), rng.standard_normal((3, below)).astype(np.float32)
    wide_c, wide_r = np.concatenate([cand, cand[:, :1]], 1), np.concatenate([rel, rel[:, :1]], 1)
    lengths = np.full(3, below, np.int32)
    a, b = _mmr(rows, cand, rel, None, 0.7, 100), _mmr(rows, wide_c, wide_r, lengths, 0.7, 100)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    (ai, av), (bi, bv) = _ils(rows, cand, None, KS), _ils(rows, wide_c, lengths, KS)
    assert np.array_equal(_bits(ai), _bits(bi)) and np.array_equal(av, bv)


def test_absent_candidates_and_their_failure_bits():
    rows, cand, rel = _exact_case(32, 65, 4, 11)
    bad_c, bad_r = cand.copy(), rel.copy()
    bad_c[1, 0], bad_c[1, 30], bad_c[2, 64] = NI, -1, 2 ** 31 - 1
    bad_r[2, 5], bad_r[3, 1], bad_r[3, 2] = np.nan, np.inf, -np.inf
    lengths = np.array([65, 65, 65, 65], np.int32)
    for c, r, bits in ((bad_c, rel, rref.FAIL_POS), (cand, bad_r, rref.FAIL_REL), (bad_c, bad_r, rref.FAIL_POS | rref.FAIL_REL)):
        want = rref.mmr_ref(rows, c, r, lengths, 0.5, 65, np.float64, [rref.gram_of(rows, x) for x in c])
        assert want[5] == bits and want[4].min() < 65
        _same_mmr(_mmr(rows, c, r, lengths, 0.5, 65, bits), want[:5])
        _same_mmr(_mmr(rows, c, r, None, 0.5, 65, bits), want[:5])
    # what lies behind a list's length is not looked at
    short = np.array([65, 0, 64, 1], np.int32)
    want = rref.mmr_ref(rows, bad_c, bad_r, short, 0.5, 65, np.float64, [rref.gram_of(rows, x) for x in bad_c])
    assert want[5] == rref.FAIL_REL
    _same_mmr(_mmr(rows, bad_c, bad_r, short, 0.5, 65, rref.FAIL_REL), want[:5])
    wi, wv, wf = rref.ils_ref(rows, bad_c, lengths, (2, 31, 65), np.float64, [rref.gram_of(rows, x) for x in bad_c])
    gi, gv = _ils(rows, bad_c, lengths, (2, 31, 65), rref.FAIL_POS)
    assert wf == rref.FAIL_POS and np.array_equal(_bits(gi), _bits(wi)) and np.array_equal(gv, wv)
    _ils(rows, bad_c, lengths, (2, 30), rref.FAIL_POS)
    _ils(rows, bad_c[2:], lengths[2:], (2, 30), 0)                              # the bad position lies behind kmax
    with pytest.raises(Exception, match="bit 30"):
        from esrecsys_amd import rerank
        rerank.mmr(_t(bad_c), _t(rel), None, _t(rows))
    with pytest.raises(Exception, match="bit 29"):
        rerank.mmr(_t(cand), _t(bad_r), None, _t(rows))


def test_ils_order_witnesses_on_the_device():
    """sims 1, 2^53, -2^53: 0 in the stated fp64 order, a different number in the reversed one -- inside one row's chain and
    across the prefix (tests/test_rerank_ref.py shows the reversed values)"""
    for rows, rev in ((rref.WITNESS_ROW_CHAIN, dict(reverse_j=True)), (rref.WITNESS_PREFIX, dict(reverse_i=True))):
        n = rows.shape[0]
        cand = np.arange(n, dtype=np.int32)[None, :]
        want = rref.ils_query(rows, cand[0], n, (n,), np.float32)[0]
        other = rref.ils_query(rows, cand[0], n, (n,), np.float32, **rev)[0]
        got, valid = _ils(rows, cand, None, (n,))
        assert want[0] == 0.0 and other[0] != 0.0 and np.array_equal(_bits(got[0]), _bits(want)) and valid.tolist() == [[1]]


# ---- independence ------------------------------------------------------------------------------------------------------------
def test_a_query_does_not_depend_on_its_batch_or_on_n_out():
    rng = np.random.default_rng(5)
    D, width, nq = 100, 257, 6
    rows = rng.standard_normal((NI, D)).astype(np.float32)
    cand, rel = rng.integers(0, NI, (nq, width)).astype(np.int32), rng.standard_normal((nq, width)).astype(np.float32)
    lengths = np.array([257, 100, 0, 1, 256, 300], np.int32)
    whole = _mmr(rows, cand, rel, lengths, 0.6, width)
    for q in range(nq):
        alone = _mmr(rows, cand[q:q + 1], rel[q:q + 1], lengths[q:q + 1], 0.6, width)
        for x, y in zip(whole, alone):
            assert np.array_equal(x[q:q + 1].view(np.uint32), y.view(np.uint32))
    for n_out in (1, 2, 100):
        short = _mmr(rows, cand, rel, lengths, 0.6, n_out)
        for x, y in zip(whole[:4], short[:4]):
            assert np.array_equal(x[:, :n_out].view(np.uint32), y.view(np.uint32))
        assert np.array_equal(short[4], np.minimum(whole[4], n_out))
    wi, wv = _ils(rows, cand, lengths, KS)
    for q in range(nq):
        ai, av = _ils(rows, cand[q:q + 1], lengths[q:q + 1], KS)
        assert np.array_equal(_bits(ai), _bits(wi[q:q + 1])) and np.array_equal(av, wv[q:q + 1])


def test_past_the_grid_cap():
    from esrecsys_amd import ops
    cap = ops.rerank_geometry(4, 3)["grid_cap"]
    rng = np.random.default_rng(6)
    rows = rng.standard_normal((50, 4)).astype(np.float32)
    base_c, base_r = rng.integers(0, 50, (11, 3)).astype(np.int32), rng.standard_normal((11, 3)).astype(np.float32)
    base_l = np.array([3, 3, 2, 0, 3, 1, 3, 3, 2, 3, 3], np.int32)
    nq = 2 * cap + 7
    idx = np.arange(nq) % 11
    small, big = _mmr(rows, base_c, base_r, base_l, 0.4, 3), _mmr(rows, base_c[idx], base_r[idx], base_l[idx], 0.4, 3)
    for x, y in zip(small, big):
        assert np.array_equal(x[idx].view(np.uint32), y.view(np.uint32))
    (si, sv), (bi, bv) = _ils(rows, base_c, base_l, (2, 3)), _ils(rows, base_c[idx], base_l[idx], (2, 3))
    assert np.array_equal(_bits(si[idx]), _bits(bi)) and np.array_equal(sv[idx], bv)


# ---- random tables: the project's bound ------------------------------------------------------------------------------------
def _keep(key, err, e32, scale):
    MEASURED[key] = {"error": err, "e32": e32, "multiple_of_e32": err / e32 if e32 else 0.0,
                     "share_of_bound": err / (rref.FACTOR * e32 + rref.FLOOR * scale)}
    path = os.environ.get("ESR_RERANK_PARITY_JSON")     # (profiles/rerank/parity_errors.json is one run written this way)
    if path:
        with open(path, "w") as f:
            json.dump(MEASURED, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("D,width,lam", [(32, 65, 0.3), (100, 257, 0.7), (128, 300, 0.5), (64, 64, 0.0), (8, 1024, 0.9)])
def test_random_tables_every_round_within_the_bound(D, width, lam):
    """a greedy rule cascades, so whole lists are not compared: every round's values are recomputed in fp64 and in the
    float32 chain from the kernel's OWN earlier picks; its pick must be the fp64 maximum within eps_t and its value the
    fp64 value within eps_t, eps_t = 4 e32_t + 2^-22 max(1, |v|), e32_t the float32 restatement's largest error of the round"""
    rng = np.random.default_rng(D + width)
    nq = 3
    rows = (rng.standard_normal((NI, D)) / np.sqrt(D)).astype(np.float32)
    cand, rel = rng.integers(0, NI, (nq, width)).astype(np.int32), rng.standard_normal((nq, width)).astype(np.float32)
    lengths = np.array([width, (2 * width) // 3, width], np.int32)
    n_out = min(width, 130)
    pos, item, orel, value, length = _mmr(rows, cand, rel, lengths, lam, n_out)
    worst = (0.0, 0.0, 1.0, 0.0)
    for q in range(nq):
        assert length[q] == min(n_out, lengths[q]) and len(set(pos[q, :length[q]].tolist())) == length[q]
        picks = pos[q, :length[q]]
        assert np.array_equal(item[q, :length[q]], cand[q, picks]) and np.array_equal(_bits(orel[q, :length[q]]), _bits(rel[q, picks]))
        v64 = rref.mmr_query(rows, cand[q], rel[q], lengths[q], lam, n_out, np.float64, picks=picks)["values"]
        v32 = rref.mmr_query(rows, cand[q], rel[q], lengths[q], lam, n_out, np.float32, picks=picks)["values"]
        for t, s in enumerate(picks):
            live = np.isfinite(v64[t])
            assert live[s]
            e32 = float(np.abs(v32[t][live].astype(np.float64) - v64[t][live]).max())
            scale = max(1.0, float(np.abs(v64[t][live]).max()))
            eps = rref.FACTOR * e32 + rref.FLOOR * scale
            err = abs(float(value[q, t]) - float(v64[t][s]))
            assert v64[t][s] >= v64[t][live].max() - eps, (q, t)
            assert err <= eps, (q, t, err, eps)
            if err / eps > worst[3]:
                worst = (err, e32, scale, err / eps)
    print("mmr D=%d width=%d lam=%g: worst round error %.3g, e32 %.3g, share of the bound %.3g" % ((D, width, lam) + worst[:2] + worst[3:]))
    _keep("mmr_value_D%d_w%d" % (D, width), *worst[:3])


@pytest.mark.parametrize("D,width", [(32, 65), (100, 257), (128, 300), (8, 1024)])
def test_random_tables_ils_within_the_bound(D, width):
    rng = np.random.default_rng(D * width)
    rows = (rng.standard_normal((NI, D)) / np.sqrt(D)).astype(np.float32)
    cand = rng.integers(0, NI, (3, width)).astype(np.int32)
    lengths = np.array([width, width // 2, 5], np.int32)
    ks = (2, 10, 100, 2000)
    got, valid = _ils(rows, cand, lengths, ks)
    w64, v64, _ = rref.ils_ref(rows, cand, lengths, ks, np.float64)
    w32, _, _ = rref.ils_ref(rows, cand, lengths, ks, np.float32)
    assert np.array_equal(valid, v64) and valid.all()
    e32 = float(np.abs(w32.astype(np.float64) - w64).max())
    err = float(np.abs(got.astype(np.float64) - w64).max())
    scale = max(1.0, float(np.abs(w64).max()))
    print("ils D=%d width=%d: error %.3g, e32 %.3g" % (D, width, err, e32))
    assert err <= rref.FACTOR * e32 + rref.FLOOR * scale
    _keep("ils_D%d_w%d" % (D, width), err, e32, scale)


# ---- model level ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """two tight item clusters (ids 100.. and 200.., 12 items each) around orthogonal directions a and b; every user is
    a + 0.8 b, so all of cluster A outscores all of cluster B"""
    import torch
    from esrecsys_amd.factorization import BPR
    rng = np.random.default_rng(9)
    D, per, nu = 16, 12, 12
    item_ids = np.concatenate([100 + np.arange(per), 200 + np.arange(per)])
    user = np.repeat(np.arange(nu), 2)
    item = np.concatenate([[item_ids[u % per], item_ids[per + u % per]] for u in range(nu)])
    model = BPR(user, item, rank=D, seed=0)
    a, b = np.eye(D, dtype=np.float32)[0], np.eye(D, dtype=np.float32)[1]
    Y = np.concatenate([a + 0.02 * rng.standard_normal((per, D)), b + 0.02 * rng.standard_normal((per, D))]).astype(np.float32)
    X = np.tile(a + 0.8 * b, (nu, 1)).astype(np.float32)
    assert np.array_equal(model.items.cpu().numpy(), item_ids)
    model.item_factors.copy_(torch.from_numpy(Y))
    model.user_factors.copy_(torch.from_numpy(X))
    return model, np.arange(nu), X, Y, item_ids, per


def test_diversify_mixes_the_clusters_and_lowers_ils(planted):
    """recommend's top 10 is cluster A alone (scores about 1 against 0.8).  On unit rows at lam = 0.5: after the first A the
    other A's are worth 0.5 * 1 - 0.5 * 1 = 0 and the B's 0.5 * 0.8 - 0 = 0.4, so a B comes second; from then on an A is
    worth 0 and a B 0.4 - 0.5 = -0.1: nine A's and one B.  ILS@10 falls from about 1 (45 pairs inside A) to about 36 / 45 =
    0.8 (the nine pairs with the B are about 0)."""
    import torch
    from esrecsys_amd import rerank
    model, users, X, Y, item_ids, per = planted
    ids, scores, lengths = model.recommend(users, k=24, exclude_seen=False)
    top = ids[:, :10].cpu().numpy()
    assert (top < 200).all() and lengths.tolist() == [24] * len(users)          # ten of cluster A
    d_ids, d_scores, d_len = model.diversify(ids, scores, lengths, lam=0.5, n=10)
    got = d_ids.cpu().numpy()
    assert d_ids.shape == (len(users), 10) and d_len.tolist() == [10] * len(users)
    assert ((got < 200).sum(1) == 9).all() and ((got >= 200).sum(1) == 1).all() and (got[:, 1] >= 200).all()
    # the fp64 restatement on the host shows the same lists
    rows = rerank.unit_rows(model.item_factors)
    unit = rows.cpu().numpy()
    assert np.abs((unit.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6
    pos = np.searchsorted(item_ids, ids.cpu().numpy())
    for q in range(len(users)):
        r = rref.mmr_query(unit, pos[q], scores[q].cpu().numpy(), 24, 0.5, 10, np.float64)
        assert np.array_equal(item_ids[r["item"]], got[q])
    before = rerank.intra_list_similarity(model._positions(ids.reshape(-1), model.items).reshape(ids.shape), lengths, rows, ks=(10,))
    after = rerank.intra_list_similarity(model._positions(d_ids.reshape(-1), model.items).reshape(d_ids.shape), d_len, rows, ks=(10,))
    b, a = before.mean(), after.mean()
    assert b["n_valid"].tolist() == [len(users)] and a["ils"][0] < 0.85 < 0.95 < b["ils"][0]
    # every user is the same vector: one list of ten distinct ids before and after, eleven over the two together
    assert rerank.coverage(d_ids, d_len, (10,))[0] == 10 == rerank.coverage(ids, lengths, (10,))[0]
    assert rerank.coverage(torch.cat([ids[:, :10], d_ids]), None, (10,))[0] == 11
    with pytest.raises(ValueError, match="query 1: id 999"):
        bad = ids.clone()
        bad[1, 2] = 999
        model.diversify(bad, scores, lengths)
    bad_len = lengths.clone()
    bad_len[1] = 2
    model.diversify(bad, scores, bad_len, n=2)                                    # behind the length: not looked at


def test_diversify_at_lam_one_is_recommend_and_feeds_the_metrics(planted):
    from esrecsys_amd.evaluate import ranking_metrics
    model, users, X, Y, item_ids, per = planted
    ids, scores, lengths = model.recommend(list(users) + [777], k=20)            # an unknown user: an empty list
    assert lengths.tolist() == [20] * len(users) + [0]
    for n in (7, 20):
        d_ids, d_scores, d_len = model.diversify(ids, scores, lengths, lam=1.0, n=n, normalize=False)
        assert np.array_equal(d_ids.cpu().numpy(), ids[:, :n].cpu().numpy())
        assert np.array_equal(_bits(d_scores.cpu().numpy()), _bits(scores[:, :n].cpu().numpy()))
        assert d_len.tolist() == [n] * len(users) + [0] and d_ids.dtype == ids.dtype and d_scores.dtype == scores.dtype
    truth = np.concatenate([[item_ids[(u + 1) % per], item_ids[per + (u + 3) % per]] for u in users] + [[100]]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([2] * len(users) + [1])]).astype(np.int64)
    same = ranking_metrics(d_ids, d_len, truth, offsets, ks=(10, 20)).mean()
    base = ranking_metrics(ids, lengths, truth, offsets, ks=(10, 20)).mean()
    assert same["n_valid"] == base["n_valid"] and np.array_equal(same["recall"], base["recall"])
    mixed = model.diversify(ids, scores, lengths, lam=0.5, n=10)
    m = ranking_metrics(mixed[0], mixed[2], truth, offsets, ks=(10,)).mean()
    assert 0.0 <= m["recall"][0] <= 1.0 and np.isfinite(m["ndcg"][0])

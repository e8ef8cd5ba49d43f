"""CPU: the NumPy helper behind tests/test_gpu_inbatch_step_oracle.py (tests/_inbatch_step_ref.py) -- it is the oracle
chain and nothing else, its id builder puts the runs of the sorted occurrence list where a spec says, every case of the
GPU test finds a seed that keeps the input conditions, and its comparison accepts an f32 evaluation and refuses each of
ten wrong steps (the mutants (a) to (j) below), every one built from the fp64 reference and rounded to the table types."""
import numpy as np
import pytest

import _inbatch_step_ref as R
from oracle import optim as o_optim
from oracle import stl_head as o_stl

F64 = np.float64


def test_step_ref_is_the_oracle_chain():
    """two steps on small towers: the oracle calls written out, against step_ref"""
    rng = np.random.default_rng(5)
    q, c = rng.standard_normal((9, 6)) * 0.6, rng.standard_normal((11, 6)) * 0.6
    qa, ca = rng.uniform(0.01, 1, q.shape), rng.uniform(0.01, 1, c.shape)
    for step in range(2):
        qid, cid = rng.integers(0, 9, 8), rng.integers(0, 11, 8)
        loss, lse, gq, gc = o_stl.inbatch_softmax_loss_and_grads(q[qid], c[cid], 0.1, 12.0, 5.0, F64)
        q2, qa2 = o_optim.sparse_adagrad_update(q, qa, qid, gq, 0.05, 1e-7, dtype=F64)
        c2, ca2 = o_optim.sparse_adagrad_update(c, ca, cid, gc, 0.05, 1e-7, dtype=F64)
        r = R.step_ref(q, c, qa, ca, qid, cid, 5.0, 0.1, 12.0, 0.05, 1e-7, F64)
        assert r["loss"] == loss and np.array_equal(r["lse"], lse)
        for k, want in zip(R.ARRAYS, (q2, c2, qa2, ca2)):
            assert np.array_equal(r[k], want)
        assert np.array_equal(np.flatnonzero(r["touched_query"]), np.unique(qid))
        assert np.array_equal(np.flatnonzero(r["touched_cand"]), np.unique(cid))
        # rows nobody names keep their bits, the others move
        assert np.array_equal(r["query"][~r["touched_query"]], q[~r["touched_query"]])
        assert not np.any(r["cand_acc"][r["touched_cand"]] == ca[r["touched_cand"]])
        q, c, qa, ca = q2, c2, qa2, ca2


def test_ids_with_layout_puts_the_runs_where_they_are_asked_for():
    rng = np.random.default_rng(3)
    ids = R.ids_with_layout(300, 200, [(31, 32), (100, 5), (195, 5)], rng, fill=(1, 2, 3))
    assert ids.dtype == np.int32 and ids.shape == (200,) and ids.min() >= 0 and ids.max() < 300
    assert np.any(np.diff(ids) < 0)  # shuffled: the occurrences of a run are spread over the batch
    srt = np.sort(ids)
    for start, length in ((31, 32), (100, 5), (195, 5)):
        assert np.all(srt[start:start + length] == srt[start]) and (start == 0 or srt[start - 1] != srt[start])
        assert start + length == 200 or srt[start + length] != srt[start]
    assert set(R.run_lengths(np.concatenate([srt[:31], srt[63:100]])).values()) <= {1, 2, 3}
    pooled = R.ids_with_layout(300, 64, [(16, 5)], rng, id_pool=np.arange(300))
    assert np.array_equal(np.unique(pooled), np.arange(np.unique(pooled).size))
    with pytest.raises(AssertionError):
        R.ids_with_layout(10, 200, [], rng, fill=(1,))


@pytest.mark.parametrize("D", R.GEOMETRY_WIDTHS)
def test_geometry_cases_have_their_run_structure(D):
    """run start modulo 32, run length and tower of every named family, from the helper's own stable argsort"""
    def runs(name):
        c = R.make_case("%s-D%d" % (name, D))
        return c, R.asked_runs(c), R.sorted_runs(c)
    c, asked, every = runs("distinct")
    assert not asked and len(every) == 2 * c.B and not R.has_long_run(c)
    c, _, every = runs("runs2to31")
    lengths = {r[1] for r in every}
    assert min(lengths) >= 2 and max(lengths) == 31 and {2, 31} <= lengths and not R.has_long_run(c)
    for name, mod in (("run32-a0", 0), ("run32-a1", 1), ("run32-a31", 31)):
        c, asked, every = runs(name)
        assert [(s % 32, n, t) for s, n, t, _ in asked] == [(mod, 32, 0), (mod, 32, 1)]
        assert R.longest_run(c) == 32 and not R.has_long_run(c)  # exactly a chunk: still no long run
    c, asked, _ = runs("run33-64")
    assert sorted((n, t) for _, n, t, _ in asked) == [(33, 0), (33, 1), (64, 0), (64, 1)] and R.has_long_run(c)
    for name, towers in (("hot-q", [0]), ("hot-c", [1]), ("hot-both", [0, 1])):
        c, asked, every = runs(name)
        assert [(n, t) for _, n, t, _ in asked] == [(n, t) for t in towers for n in (65, 70, 300)]
        assert all(n <= 13 for _, n, t, _ in every if t not in towers) and R.has_long_run(c)
        assert asked[0][0] % 32 == 3 and asked[0][0] // 32 + 2 == (asked[0][0] + 64) // 32  # 65: head chunk + two more
    for name, long in (("edges", False), ("edges-long", True)):
        c, asked, every = runs(name)
        ends = [(s + n, t) for s, n, t, _ in asked]
        assert (c.B, 0) in ends and (2 * c.B, 1) in ends and (c.B, 1) in [(s, t) for s, _, t, _ in asked]
        assert every[-1] == asked[-1] and R.has_long_run(c) == long
    c, asked, _ = runs("same-id")
    (_, nq, tq, iq), (_, nc, tc, ic) = asked
    assert (nq, tq, nc, tc) == (5, 0, 9, 1) and iq == ic  # one number, a row of each tower
    assert (c.qid == iq).sum() == 5 and (c.cid == iq).sum() == 9 and max(c.qid.max(), c.cid.max()) < c.Vq
    assert R.make_case("negscale-D%d" % D).scale < 0 and R.make_case("eps-D%d" % D).eps == R.BIG_EPS
    c = R.make_case("biglr-D%d" % D)
    moved = R.arr_err(c.reference().r64["query"], c.query)
    print("biglr-D%d: the query tower moves by %.3f of its largest entry in the step" % (D, moved))
    assert c.lr == R.BIG_LR and moved > 0.01


def test_shape_cases_cover_the_batches_and_widths():
    seen = {(s.B, s.D) for s in (R.SPECS[n] for n in R.SHAPE_CASES)}
    assert seen == {(B, D) for B in R.BATCHES for D in R.WIDTHS if D == 128 or B in (256, 1024)}
    assert {R.SPECS[n].scale for n in R.SHAPE_CASES} == {4.0, 5.0, 6.0, 7.0, 8.0}
    assert all(R.SPECS[n].batch_size == 1.5 * R.SPECS[n].B for n in R.SHAPE_CASES)
    assert 2 * max(R.BATCHES) >= 4096 > 2 * sorted(R.BATCHES)[-2] and {128 % 256, 384 % 256} == {128}
    assert all(D % 4 == 0 and B % 128 == 0 for B, D in seen)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(R.SPECS))
def test_every_case_finds_a_seed_that_keeps_the_input_conditions(name, dtype):
    case = R.make_case(name, dtype)  # raises when none of the 20 seeds does
    gap, both = R.input_conditions(case)
    ref = case.reference()
    print("%s/%s: seed %d, min ||row| - 1| %.3g, longest run %d, loss %.6g" % (name, dtype, case.seed, gap,
                                                                            R.longest_run(case), ref.r64["loss"]))
    assert gap >= R.MIN_NORM_GAP and both and R.make_case(name, dtype) is case  # computed once
    assert all(np.all(np.isfinite(ref.r64[k])) for k in R.BOUNDED)
    assert case.batch_size != case.B and case.qid.shape == case.cid.shape == (case.B,)
    assert 0 <= case.qid.min() and case.qid.max() < case.Vq and 0 <= case.cid.min() and case.cid.max() < case.Vc
    for a in (case.query_acc, case.cand_acc):  # accumulators are not constant
        assert a.dtype == np.float32 and 0.01 <= a.min() < 0.05 and 0.9 < a.max() <= 1.0
    assert not ref.touched["query"].all() and not ref.touched["cand"].all()  # some rows nobody names
    if dtype == "bf16":
        assert np.array_equal(o_optim.round_bf16(case.query), case.query)
        assert max(ref.tie_fraction.values()) < R.MAX_TIE_FRACTION


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("a,b", [("ws-big-D128", "ws-small-D128"), ("ws-small-D128", "ws-big-D128")])
def test_second_step_case_keeps_the_input_conditions(a, b, dtype):
    first = R.make_case(a, dtype).reference()
    case = R.make_second_step(first, b)
    gap, both = R.input_conditions(case)
    assert gap >= R.MIN_NORM_GAP and both and case.B == R.SPECS[b].B != first.case.B
    for got, k in zip(case.inputs(), R.ARRAYS):  # the towers the first step leaves, in the table's type
        want = first.r64[k]
        if dtype == "bf16" and k in R.TOWERS:
            want = o_optim.round_bf16(want)
        assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    again = R.with_inputs(case, *first.case.inputs())
    assert again.query is first.case.query and again.qid is case.qid


# ---- the comparison: accepts the f32 oracle, refuses ten wrong steps -------------------------------------------------------
def _as_got(case, r):
    got = {k: np.asarray(r[k]).astype(np.float32) for k in R.ARRAYS}
    if case.dtype == "bf16":
        for k in R.TOWERS:
            got[k] = R.bf16_bits(o_optim.round_bf16(r[k]))
    return got


def _compare(case, r):
    return R.compare(case.reference(), _as_got(case, r), np.float32(r["loss"]), np.asarray(r["lse"]).astype(np.float32))


def _refused(case, r, *arrays):
    """compare() names every one of `arrays` among its failures"""
    _, fails = _compare(case, r)
    assert all(any(f.startswith(k + ":") for f in fails) for k in arrays), (case.spec.name, case.dtype, arrays, fails)


def _grads(case, query=None):
    q = (case.query if query is None else query).astype(F64)
    return o_stl.inbatch_softmax_loss_and_grads(q[case.qid], case.cand.astype(F64)[case.cid], case.lam, case.batch_size,
                                                case.scale, F64)[2:]


def _adagrad(case, param, accum, ids, rows, squares_of_sum=True, eps_inside=True):
    """oracle.optim.sparse_adagrad_update with the two places a wrong step differs in"""
    uniq, g = o_optim.segment_sum_rows(ids, rows, F64)
    sq = g * g if squares_of_sum else o_optim.segment_sum_rows(ids, rows * rows, F64)[1]
    p, a = param.astype(F64).copy(), accum.astype(F64).copy()
    acc = a[uniq] + sq
    p[uniq] -= case.lr * g / (np.sqrt(acc + case.eps) if eps_inside else np.sqrt(acc) + case.eps)
    a[uniq] = acc
    return p, a


def _with(case, **arrays):
    r = dict(case.reference().r64)
    r.update(arrays)
    return r


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["shape-B256-D4", "shape-B1024-D100", "shape-B2176-D128", "hot-both-D128", "biglr-D64",
                                  "negscale-D128"])
def test_compare_accepts_the_f32_oracle(name, dtype):
    case = R.make_case(name, dtype)
    ratios, fails = _compare(case, case.ref(np.float32))
    assert not fails and max(ratios.values()) <= 0.25 + 1e-12
    ratios, fails = _compare(case, case.ref(F64))
    assert not fails and max(ratios.values()) <= 0.25  # the f32 storage of the exact result: 2^-24, inside the floor
    mine = _adagrad(case, case.query, case.query_acc, case.qid, _grads(case)[0])  # (the mutants' own update, unmutated)
    assert all(np.allclose(a, case.reference().r64[k], rtol=1e-13, atol=0) for a, k in zip(mine, ("query", "query_acc")))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["run32-a0-D128", "run32-a31-D64"])
@pytest.mark.parametrize("mutant", ["a", "b", "c"])
def test_a_wrong_run_sum_is_refused(mutant, name, dtype):
    """(a) one occurrence of a run of 32 left out; (b) the last occurrence of the run counted twice; (c) Adagrad fed the sum
    of the squares of the occurrences instead of the square of their sum -- in either tower"""
    case = R.make_case(name, dtype)
    gq, gc = _grads(case)
    for (_, n, tower, row), ids, g, k in zip(R.asked_runs(case), (case.qid, case.cid), (gq, gc), R.TOWERS):
        occ = np.flatnonzero(ids == row)
        assert n == occ.size == 32 and k == R.TOWERS[tower]
        use = {"a": np.delete(np.arange(case.B), occ[7]), "b": np.append(np.arange(case.B), occ[-1]),
               "c": np.arange(case.B)}[mutant]
        p, a = _adagrad(case, getattr(case, k), getattr(case, k + "_acc"), ids[use], g[use], squares_of_sum=mutant != "c")
        _refused(case, _with(case, **{k: p, k + "_acc": a}), k, k + "_acc")
        _refused(case, _with(case, **{k: p}), k)  # (the row alone, the accumulator right)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_an_unwritten_accumulator_is_refused(dtype):
    """(d), where it shows least: every id occurs once"""
    case = R.make_case("distinct-D128", dtype)
    _refused(case, _with(case, query_acc=case.query_acc), "query_acc")
    _refused(case, _with(case, cand_acc=case.cand_acc), "cand_acc")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", R.GEOMETRY_WIDTHS)
def test_candidate_gradients_from_updated_query_rows_are_refused(D, dtype):
    """(e) the hazard the overlapped form's row copies exist for; the large learning rate is what makes it show"""
    case = R.make_case("biglr-D%d" % D, dtype)
    moved = case.reference().next_inputs()[0]  # the query tower after its update, as its table holds it
    gc = _grads(case, query=moved)[1]
    p, a = _adagrad(case, case.cand, case.cand_acc, case.cid, gc)
    _refused(case, _with(case, cand=p, cand_acc=a), "cand", "cand_acc")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["shape-B256-D128", "shape-B1024-D32"])
def test_wrong_settings_are_refused(name, dtype):
    """(f) the regulariser's term dropped, (g) B used where batch_size belongs"""
    case = R.make_case(name, dtype)
    no_reg = case.ref(F64, lam=0.0)
    _refused(case, no_reg, "loss", "query", "cand")
    _refused(case, _with(case, **{k: no_reg[k] for k in R.ARRAYS}), "query", "cand")  # (in the gradients only)
    _refused(case, case.ref(F64, batch_size=float(case.B)), "loss", "query", "cand", "query_acc", "cand_acc")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", R.GEOMETRY_WIDTHS)
def test_the_other_towers_row_is_refused(D, dtype):
    """(h) the candidate tower's occurrences applied to the QUERY rows of the same numbers (the virtual-row offset lost)"""
    case = R.make_case("same-id-D%d" % D, dtype)
    gq, gc = _grads(case)
    p, a = _adagrad(case, case.query, case.query_acc, np.concatenate([case.qid, case.cid]), np.concatenate([gq, gc]))
    _refused(case, _with(case, query=p, query_acc=a, cand=case.cand, cand_acc=case.cand_acc), *R.ARRAYS)
    # only the one row that the spec names in both towers
    row = R.asked_runs(case)[0][3]
    r = case.reference().r64
    mixed = {k: r[k].copy() for k in R.ARRAYS}
    for k in ("query", "query_acc"):
        mixed[k][row] = (p if k == "query" else a)[row]
    for k in ("cand", "cand_acc"):
        mixed[k][row] = getattr(case, k)[row]
    _refused(case, _with(case, **mixed), *R.ARRAYS)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", R.GEOMETRY_WIDTHS)
def test_eps_outside_the_square_root_is_refused(D, dtype):
    """(i)"""
    case = R.make_case("eps-D%d" % D, dtype)
    gq, gc = _grads(case)
    _refused(case, _with(case, query=_adagrad(case, case.query, case.query_acc, case.qid, gq, eps_inside=False)[0]), "query")
    _refused(case, _with(case, cand=_adagrad(case, case.cand, case.cand_acc, case.cid, gc, eps_inside=False)[0]), "cand")


@pytest.mark.parametrize("name", ["shape-B256-D128", "shape-B256-D4"])
def test_truncated_bf16_results_are_refused(name):
    """(j) bf16 results truncated instead of rounded to nearest even"""
    case = R.make_case(name, "bf16")
    ref = case.reference()
    got = _as_got(case, ref.r64)
    for k in R.TOWERS:
        got[k] = (np.ascontiguousarray(ref.r64[k].astype(np.float32)).view(np.uint32) >> 16).astype(np.uint16)
    _, fails = R.compare(ref, got, ref.r64["loss"], ref.r64["lse"])
    assert len(fails) == 2 and fails[0].startswith("query:") and fails[1].startswith("cand:")
    # one element, one bf16 ulp, as far from a tie as its row gets
    got = _as_got(case, ref.r64)
    row = int(case.cid[0])
    got["cand"][row, int(np.argmax(R.midpoint_distance(ref.r64["cand"][row])))] ^= 1
    _, fails = R.compare(ref, got, ref.r64["loss"], ref.r64["lse"])
    assert len(fails) == 1 and fails[0].startswith("cand:")

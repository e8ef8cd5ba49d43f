"""CPU: the NumPy helper behind tests/test_gpu_glove_step_oracle.py (tests/_glove_step_ref.py) -- it is the oracle chain
the existing trajectory test uses, every case of the GPU test builds with its input conditions, run structure and reached
kernel instantiation, and its comparison accepts an f32 evaluation and refuses every wrong step tried here."""
import numpy as np
import pytest

import _glove_step_ref as R
from oracle import glove as o_glove
from oracle import optim as o_optim


def test_step_ref_is_the_oracle_chain_of_the_trajectory_test():
    """the oracle calls of test_fused_step_trajectory_vs_fp64_oracle, written out, against step_ref"""
    rng = np.random.default_rng(3)
    V, D, B, lr = 70, 12, 64, 0.05
    emb, bias = rng.standard_normal((V, D)) / np.sqrt(D), 0.05 * rng.standard_normal((V, 1))
    a_e, a_b = np.full_like(emb, 0.1), np.full_like(bias, 0.1)
    for mode in R.MODES:
        inputs = rng.integers(0, V, (2, B)).astype(np.int32)
        target = rng.uniform(0.1, 300.0, B)
        el, gdot, gs = o_glove.loss_and_grads(emb, bias, inputs, target, mode, np.float64)
        ids, rows, gb = o_glove.row_grads(emb, inputs, gdot, gs, np.float64)
        e2, ae2 = o_optim.sparse_adagrad_update(emb, a_e, ids, rows, lr, dtype=np.float64)
        b2, ab2 = o_optim.sparse_adagrad_update(bias, a_b, ids, gb[:, None], lr, dtype=np.float64)
        r = R.step_ref(emb, a_e, bias[:, 0], a_b[:, 0], inputs, target, mode, lr, 1e-7, np.float64)
        assert r["loss"] == el
        for k, want in zip(R.KEYS, (e2, ae2, b2[:, 0], ab2[:, 0])):
            assert np.array_equal(r[k], want)
        untouched = np.setdiff1d(np.arange(V), inputs.reshape(-1))
        assert untouched.size and np.array_equal(r["emb"][untouched], emb[untouched])


def test_geometry_mirror_and_the_instantiations_the_widths_reach():
    assert [R.row_geom(D) for D in (4, 128, 260, 1024, 1028, 6, 255, 257)] == [
        (4, 1, 1, 1), (4, 32, 32, 1), (4, 65, 64, 2), (4, 256, 64, 4), (4, 257, 64, 5), (1, 6, 8, 1), (1, 255, 64, 4),
        (1, 257, 64, 5)]
    assert R.row_geom(1024, 8) == (8, 128, 64, 2) and R.row_geom(128, 8) == (8, 16, 16, 1)
    assert all(R.dim_supported(D) for D in R.WIDTHS) and not any(R.dim_supported(D) for D in R.REFUSED_WIDTHS)
    assert max(R.WIDTHS_VEC4) == 1024 and not R.dim_supported(1028) and set(R.WIDTHS_SCALAR) >= {253, 254, 255}
    reached = {D: R.instantiation(D) for D in R.WIDTHS}
    assert {v[:2] for v in reached.values()} == {(vec, nch) for vec in (4, 1) for nch in (1, 2, 4)}
    # lane counts: one lane, a few, a whole wave -- for float4 and scalar rows
    assert {reached[D] for D in (4, 12, 100, 128, 256)} == {(4, 1, 1), (4, 1, 4), (4, 1, 32), (4, 1, 64)}
    assert {reached[D] for D in (1, 6, 63)} == {(1, 1, 1), (1, 1, 8), (1, 1, 64)}
    assert len(set(reached.values())) == 11
    # bf16 with ESR_BF16_VEC8=1: 8-element chunks where D % 8 == 0 and both buffers are 16-byte aligned
    v8 = {D: R.instantiation(D, "bf16", vec8=True) for D in R.WIDTHS_VEC8}
    assert {v[:2] for D, v in v8.items() if D % 8 == 0} == {(8, 1), (8, 2)}  # (nch 3, 4 would need D > 1024)
    assert v8[12] == R.instantiation(12) == (4, 1, 4) and 12 % 4 == 0 and 12 % 8 != 0
    assert R.instantiation(128, "bf16", vec8=True, aligned16=False) == R.instantiation(128)
    assert R.instantiation(128, "f32", vec8=True) == (4, 1, 32)


def test_dispatch_mirror_and_the_paths_the_threshold_cases_reach():
    d = lambda name, mode="reference", **kw: R.dispatch(R.SPECS[name].B, R.SPECS[name].D, mode, **kw)  # noqa: E731
    assert d("thr-B4096", planned=True, long_runs=0)["fuse_fin"] and not d("thr-B4097", planned=True, long_runs=0)["fuse_fin"]
    assert not d("thr-B4096")["fuse_fin"] and d("thr-B4096")["long_launch"]          # in-line plan: screens itself
    assert not d("thr-B4096", planned=True, long_runs=0)["long_launch"]
    assert not d("thr-B16384")["resolved"] and d("thr-B16385")["resolved"]
    assert d("walk-resolved")["resolved"] and d("walk-resolved")["walk"]
    assert not d("walk-short")["resolved"] and d("walk-short")["walk"] and not d("thr-B16384")["walk"]
    assert [d(n)["nstat"] for n in ("nstat-B1", "nstat-B255", "nstat-B257", "thr-B16385")] == [1, 1, 2, 65]
    assert d("nstat-B257", "diagonal")["nstat"] == 0 and d("thr-B16385", "diagonal")["nstat"] == 65
    assert R.RESOLVED_CASES == ["thr-B16385", "walk-resolved"]
    assert all(R.eps_for(B) == np.float32(1e-7) for B in (1, 255, 384)) and R.eps_for(4096) < 1e-9


def _check_contents(case):
    t1, t2 = case.inputs
    flat = case.inputs.reshape(-1)
    assert flat.dtype == np.int32 and flat.min() == 0 and flat.max() == case.V - 1   # id 0 and id V - 1
    assert (t1 == t2).any()                                                          # a pair of a token with itself
    assert np.intersect1d(t1, t2).size                                               # a token in both rows
    assert (case.target == 100.0).sum() >= 1


@pytest.mark.parametrize("D", R.RUN_WIDTHS)
def test_run_cases_have_their_run_structure(D):
    def runs(name):
        c = R.make_case("%s-D%d" % (name, D))
        _check_contents(c)
        return c, R.run_lengths(c.inputs.reshape(-1)), R.sorted_ids(c.inputs)
    c, r, _ = runs("ones")
    assert r.pop(0) == 2 and set(r.values()) == {1}
    c, r, _ = runs("ladder")
    assert sorted(v for v in r.values() if v > 1) == list(range(2, 33)) and max(r.values()) == 32
    c, r, s = runs("lastrun")
    assert r[c.V - 1] == 65 == max(r.values()) and s[-1] == c.V - 1 and R.hot_partials(s, c.V - 1, R.CHUNK)[0] >= 2
    for L, a in R.HOT_RUNS:
        c, r, s = runs("run%d-a%d" % (L, a))
        partials, align = R.hot_partials(s, 1, R.CHUNK)
        assert r[1] == L == max(r.values()) and align == a and max(v for k, v in r.items() if k > 1) <= 3
        # head chunk: up to the first chunk boundary at least 32 positions on; then one partial per 32 positions
        want = {(32, 0): 1, (33, 0): 2, (64, 0): 2, (65, 0): 3, (97, 0): 4,
                (32, 31): 1, (33, 31): 1, (64, 31): 2, (65, 31): 2, (97, 31): 3}[(L, a)]
        assert partials == want
        long_hint = bool(np.any(s[:-R.CHUNK] == s[R.CHUNK:]))  # what glove_plan_kernel screens for
        assert long_hint == (L > 32)
    c = R.make_case("width-D%d" % D)
    assert set(R.run_lengths(c.inputs.reshape(-1)).values()) <= {1, 2, 3}


NAMES = sorted(R.SPECS)
SMALL = [n for n in NAMES if R.SPECS[n].B <= 4097]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", SMALL)
def test_every_case_builds_with_its_input_conditions(name, dtype, mode):
    case = R.make_case(name, dtype, mode)  # raises when none of the 20 seeds keeps the conditions
    cond = R.input_conditions(case)
    print("%s/%s/%s: seed %d, %r" % (name, dtype, mode, case.seed, cond))
    assert R.conditions_hold(cond) and cond["ties"] < 0.01 and cond["contrib"] >= 0.99
    _check_contents(case)
    w = o_glove.loss_weights(case.target)[0]
    assert w.min() >= 0.01 ** 0.75 - 1e-6 and (case.B < 3 or (w.min() < 0.5 and w.max() == 1.0))
    assert case.inputs.shape == (2, case.B) and case.emb.shape == (case.V, case.D)
    stamps = case.loc >> 1
    assert not (stamps == case.stamp).any() and stamps.max() <= 127
    if case.V >= 100:
        assert 0 < (case.loc & 1).sum() < case.V and len(set(stamps.tolist())) > 20
    if dtype == "bf16":
        assert np.array_equal(o_optim.round_bf16(case.emb), case.emb)
    st = R.initial_state(case)
    one = (case.loc & 1).astype(bool)
    nan = R.NAN16 if dtype == "bf16" else R.NAN32
    assert (st.emb[0][one] == nan).all() and (st.emb[1][~one] == nan).all()      # every dead copy is poison
    live = st.live()
    assert all(np.array_equal(a, b) for a, b in zip(live, case.arrays()))


@pytest.mark.parametrize("name", [n for n in NAMES if n not in SMALL])
def test_large_cases_build_with_their_input_conditions(name):
    for dtype in ("f32", "bf16") if name in R.RESOLVED_CASES else ("f32",):
        case = R.make_case(name, dtype, "reference")
        assert R.conditions_hold(R.input_conditions(case))
        _check_contents(case)
        assert max(R.run_lengths(case.inputs.reshape(-1)).values()) <= 3


def test_second_step_and_chain_cases_keep_the_input_conditions():
    for dtype in ("f32", "bf16"):
        a = R.make_case("run97-a31-D128", dtype, "reference")
        b = R.next_case(a, "ladder-D128")
        assert b.stamp == a.stamp + 1 and R.conditions_hold(R.input_conditions(b))
        assert np.array_equal(b.loc, R.loc_after(a.loc, a.touched(), a.stamp))
        want = a.reference().r64["emb"]
        assert np.array_equal(b.emb, (o_optim.round_bf16(want) if dtype == "bf16" else want).astype(np.float32))
        cases = R.chain_cases(["run65-a0-D128", "ones-D128", "ladder-D128"], dtype, "diagonal", first_stamp=125)
        assert [c.stamp for c in cases] == [125, 126, 127]
        ref = R.chain_reference(cases)
        assert len(ref.r64["losses"]) == 3 and ref.touched.sum() > cases[0].touched().sum()
        # a chain of one step is that step's reference
        one = R.chain_reference(cases[:1])
        assert all(np.array_equal(one.r64[k], cases[0].reference().r64[k]) for k in R.KEYS)
        stamps = R.chain_loc(cases) >> 1
        assert set(stamps[cases[2].touched()].tolist()) == {127} and (cases[0].loc >> 1).max() < 125


# ---- the comparison bites -----------------------------------------------------------------------------------------------
REPRESENTATIVE = [("width-D12", "f32", "reference"), ("run65-a0-D128", "bf16", "reference"),
                  ("run65-a31-D6", "f32", "diagonal"), ("ladder-D128", "f32", "diagonal")]


def _wrong_step(case, drop=(), drop_bias=(), emb=None, mode=None, stale_sums=False):
    """fp64 step with something wrong: occurrences `drop` (indices into the 2 B occurrence list) missing from their
    row's sums, `drop_bias` from the bias sums only, another embedding table read, the other mode's formula, or
    (reference mode) the bias gradient made from the batch sums sum w r and sum w as they stood before the last pair."""
    f = np.float64
    e = (case.emb if emb is None else emb).astype(f)
    b = case.bias.astype(f)[:, None]
    loss, gdot, gs = o_glove.loss_and_grads(e, b, case.inputs, case.target.astype(f), mode or case.mode, f)
    if stale_sums:
        dot, s = o_glove.pair_terms(e, b, case.inputs, f)
        w, lt = o_glove.loss_weights(case.target.astype(f), f)
        r = lt - dot
        gs = -(2.0 / case.B ** 2) * (np.sum((w * r)[:-1]) - s * np.sum(w[:-1]))
    ids, rows, gb = o_glove.row_grads(e, case.inputs, gdot, gs, f)
    keep = np.ones(ids.size, bool)
    keep[list(drop)] = False
    keep_b = keep.copy()
    keep_b[list(drop_bias)] = False
    e2, ea2 = o_optim.sparse_adagrad_update(case.emb.astype(f), case.emb_acc.astype(f), ids[keep], rows[keep], case.lr,
                                            case.eps, dtype=f)
    b2, ba2 = o_optim.sparse_adagrad_update(b, case.bias_acc.astype(f)[:, None], ids[keep_b], gb[keep_b][:, None], case.lr,
                                            case.eps, dtype=f)
    return {"loss": loss, "emb": e2, "emb_acc": ea2, "bias": b2[:, 0], "bias_acc": ba2[:, 0]}


def _fails(case, r, edit=None):
    before = R.initial_state(case)
    after = R.state_after(case, before, r)
    if edit:
        edit(before, after)
    return R.compare(case.reference(), before, after, r["loss"])[1]


@pytest.mark.parametrize("name,dtype,mode", REPRESENTATIVE)
def test_compare_accepts_the_oracles_and_refuses_wrong_steps(name, dtype, mode):
    case = R.make_case(name, dtype, mode)
    ref = case.reference()
    before = R.initial_state(case)
    for r in (ref.r64, case.ref(np.float32)):  # stored as f32: 2^-24 of the floor 2^-22; f32 oracle: e32 of 4 e32
        ratios, fails = R.compare(ref, before, R.state_after(case, before, r), r["loss"])
        assert not fails and max(ratios.values()) <= 0.25 + 1e-12, (ratios, fails)
    flat = case.inputs.reshape(-1)
    runs = R.run_lengths(flat)
    contrib = R.occurrence_contrib(case)
    # drop one occurrence of a run -- the WEAKEST one of the batch that the input condition counts
    in_run = np.array([runs[int(i)] >= 2 for i in flat])
    ok = np.flatnonzero(in_run & (contrib >= R.MIN_CONTRIB))
    weakest = int(ok[np.argmin(contrib[ok])])
    fails = _fails(case, _wrong_step(case, drop=[weakest]))
    assert fails and any(f.startswith(("emb", "bias")) for f in fails), fails
    # ... and count one twice (the same term, the other sign)
    assert _fails(case, _wrong_step(case, drop=[int(ok[np.argsort(contrib[ok])[1]])]))
    if "run65" in name:  # drop the last chunk of the 65-run of id 1: the occurrences from the last chunk boundary on
        occ = np.flatnonzero(flat == 1)
        first = int((flat < 1).sum())
        last_cut = (first + 64) // R.CHUNK * R.CHUNK
        tail = occ[last_cut - first:]
        assert tail.size == (1 if first % R.CHUNK == 0 else 32)
        fails = _fails(case, _wrong_step(case, drop=tail.tolist()))
        assert any(f.startswith("emb") for f in fails), fails
    # read one row from its dead buffer: the partner of the first pair
    stale = case.emb.copy()
    stale[case.inputs[1, 0]] = np.nan
    assert any(f.startswith("emb") for f in _fails(case, _wrong_step(case, emb=stale)))
    # leave one touched row's byte unflipped / without the step's stamp; write an untouched row's dead copy or byte
    row = int(flat[3])
    def unflipped(before, after): after.loc[row] = before.loc[row]  # noqa: E704
    def unstamped(before, after): after.loc[row] &= 1  # noqa: E704
    assert [f for f in _fails(case, ref.r64, unflipped) if f.startswith("loc")]
    assert [f for f in _fails(case, ref.r64, unstamped) if f.startswith("loc")]
    idle = int(np.flatnonzero(~case.touched())[0])
    def dead_written(before, after): after.emb[1 - (before.loc[idle] & 1)][idle, 0] = 0  # noqa: E704
    def idle_byte(before, after): after.loc[idle] ^= 2  # noqa: E704
    def old_copy_written(before, after): after.emb[before.loc[row] & 1][row, -1] ^= 1  # noqa: E704
    assert [f for f in _fails(case, ref.r64, dead_written) if f.startswith("emb buffer")]
    assert [f for f in _fails(case, ref.r64, idle_byte) if f.startswith("loc")]
    assert [f for f in _fails(case, ref.r64, old_copy_written) if f.startswith("emb buffer")]
    # the new value left in the buffer the row was read from (and the other one untouched)
    def not_moved(before, after):  # noqa: E306
        b = before.loc[row] & 1
        after.emb[b][row], after.emb[1 - b][row] = after.emb[1 - b][row].copy(), before.emb[1 - b][row]
    assert _fails(case, ref.r64, not_moved)
    # the bias table
    if mode == "reference":  # stepped with the batch sums as they stood before the last pair
        fails = _fails(case, _wrong_step(case, stale_sums=True))
    else:                    # a run's bias sum without its last occurrence
        fails = _fails(case, _wrong_step(case, drop_bias=[int(np.flatnonzero(flat == flat[weakest])[-1])]))
    assert fails and all(f.startswith("bias") for f in fails), fails
    # the other mode's formula
    other = R.MODES[1 - R.MODES.index(mode)]
    fails = _fails(case, _wrong_step(case, mode=other))
    assert {f.split(":")[0].split("/")[0] for f in fails} >= {"loss", "emb", "bias"}, fails
    # one element off by 8 units of the floor / one bf16 ulp away from a tie
    r = {k: np.array(v, copy=True) for k, v in ref.r64.items() if k in R.KEYS + ("loss",)}
    if dtype == "bf16":
        col = int(np.argmax(R.midpoint_distance(r["emb"][row])))
        def one_ulp(before, after): after.emb[1 - (before.loc[row] & 1)][row, col] ^= 1  # noqa: E704
        fails = _fails(case, ref.r64, one_ulp)
    else:
        r["emb"][row, 0] += 8 * R.FLOOR * np.abs(r["emb"]).max()
        fails = _fails(case, r)
    assert fails and all(f.startswith("emb") for f in fails), fails


def test_bf16_tie_rule_is_per_row():
    case = R.make_case("width-D12", "bf16", "reference")
    ref = case.reference()
    assert 0 < ref.tie_fraction < R.MAX_TIE_FRACTION
    r, c = (int(v) for v in np.argwhere(ref.near_tie & ref.touched[:, None])[0])
    before = R.initial_state(case)
    after = R.state_after(case, before, ref.r64)
    x = ref.r64["emb"][r, c]
    lo, hi = sorted((R.bits_to_f64(ref.expect_bits[r, c]), R.bits_to_f64(ref.expect_bits[r, c] ^ 1)))
    other = ref.expect_bits[r, c] + (1 if abs(R.bits_to_f64(ref.expect_bits[r, c] + 1) - x) <
                                     abs(R.bits_to_f64(ref.expect_bits[r, c] - 1) - x) else -1)
    after.emb[1 - (before.loc[r] & 1)][r, c] = other  # the neighbour on the other side of the tie: accepted
    assert not R.compare(ref, before, after, ref.r64["loss"])[1], (lo, hi, x)

"""GPU: ONE step of the one-pass Shop-The-Look train step (esr_triplet_step.hip) against the fp64 oracle
(tests/_triplet_step_ref.py: oracle.stl_head.triplet_loss_and_grads + oracle.optim.sparse_adagrad_update), on every
path the unit dispatches: every (VEC, NCH) instantiation and lane count, f32 and bf16 towers, the modes direct,
ESR_TRIPLET_DIRECT_LANES=few, ESR_TRIPLET_STEP=stamped and ESR_BF16_VEC8=1, the three run classes (1, 2..8, longer)
with their edges, a grid-stride batch and a second step on a used plan buffer.

Bounds (worked out per case, see the helper): kernel error against fp64 <= 4 e32 + 2^-22 for both towers, both
accumulators and the loss, e32 = the same oracle in float32.  bf16 towers: bit-equal to round_bf16(fp64 result) except
one bf16 ulp where the fp64 value is within that distance of a tie.  Exact in every case: rows no id names, and 64
sentinel rows of NaN bits in front of and behind every table and accumulator, keep their bits.  Input conditions
(every |margin| >= 1e-3, every | |row| - 1 | >= 1e-3) are asserted on the fp64 reference by the helper's make_case.

Largest error / bound seen per mode on an MI355X (printed at the end of a run with -s; bf16 towers have no ratio, they
are compared bit for bit):
    direct  f32   loss 0.114  scene 0.114  product 0.119  scene_acc 0.160  product_acc 0.122
    few     f32   loss 0.105  scene 0.106  product 0.119  scene_acc 0.114  product_acc 0.114
    stamped f32   loss 0.114  scene 0.108  product 0.119  scene_acc 0.160  product_acc 0.114
    direct  bf16  loss 0.384                              scene_acc 0.114  product_acc 0.114
    vec8    bf16  loss 0.082                              scene_acc 0.114  product_acc 0.114
No mode needs more than 0.4 of the bound: the step's arithmetic is an f32 evaluation of the oracle's on every path.
"""
import numpy as np
import pytest
import torch

import _triplet_step_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                     # sentinel rows in front of and behind every table
NAN32, NAN16 = 0x7FC0BEEF, 0x7FC1
_MODE_ENV = {"direct": {}, "few": {"ESR_TRIPLET_DIRECT_LANES": "few"}, "stamped": {"ESR_TRIPLET_STEP": "stamped"},
             "vec8": {"ESR_BF16_VEC8": "1"}}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for key in sorted(_WORST):
        print("\nlargest error / (4 e32 + 2^-22), %s: %s" % (key, ", ".join("%s %.3f" % kv for kv in sorted(_WORST[key].items()))))


def _set_mode(monkeypatch, mode):
    for var in ("ESR_TRIPLET_STEP", "ESR_TRIPLET_DIRECT_LANES", "ESR_BF16_VEC8", "ESR_STL_FUSED"):
        monkeypatch.delenv(var, raising=False)
    for var, val in _MODE_ENV[mode].items():
        monkeypatch.setenv(var, val)


def _reference(name, dtype):
    """fp64 / f32 oracle of a case, computed once for every mode that runs it (the input conditions are asserted by
    make_case, before any GPU work)"""
    return R.make_case(name, dtype).reference()


class Tables:
    """the four arrays of a case on the device, each a [V, D] view between PAD sentinel rows of a larger buffer"""

    def __init__(self, case, dev):
        self.case, self.bufs, self.views = case, {}, {}
        for k, a in zip(R.ARRAYS, case.inputs()):
            bf16 = case.dtype == "bf16" and k in ("scene", "product")
            V, D = a.shape
            buf = torch.empty((V + 2 * PAD, D), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
            if bf16:
                buf.view(torch.int16).fill_(NAN16)
            else:
                buf.view(torch.int32).fill_(NAN32)
            view = buf[PAD:PAD + V]
            view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev))  # (bf16 cases hold bf16 values: exact)
            assert view.is_contiguous() and view.data_ptr() % 16 == 0
            self.bufs[k], self.views[k] = buf, view
        self.before = self.raw()
        for k, a in zip(R.ARRAYS, case.inputs()):  # the upload was exact
            assert np.array_equal(self.values(self.before)[k], a if a.dtype == np.float32 else a.astype(np.float32))

    def raw(self):
        return {k: b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32).cpu().numpy() for k, b in self.bufs.items()}

    @staticmethod
    def values(raw):
        """f32 values of the [V, D] views"""
        out = {}
        for k, r in raw.items():
            v = r[PAD:-PAD]
            out[k] = (v.astype(np.uint16).astype(np.uint32) << 16).view(np.float32) if v.dtype == np.int16 else v.view(np.float32)
        return out

    def step(self, mode, monkeypatch, **kw):
        """one step through ops.triplet_train_step (stamped: through TrainState + train_step); returns the loss"""
        from esrecsys_amd import ops
        c, v, dev = self.case, self.views, self.views["scene"].device
        ids = [torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in (c.sid, c.pid, c.nid)]
        _set_mode(monkeypatch, mode)
        if mode == "stamped":
            from esrecsys_amd import TrainState, optim
            from esrecsys_amd.pinterest.train_shop_the_look import fused_triplet_step_available, train_step
            tree = lambda s, p: {"params": {"scene_tower": {"embedding": s}, "product_tower": {"embedding": p}}}  # noqa: E731
            state = TrainState(step=0, apply_fn=None, params=tree(v["scene"], v["product"]), tx=optim.sparse_adagrad(c.lr),
                               opt_state={"sum_of_squares": tree(v["scene_acc"], v["product_acc"])})
            assert state.tx.eps == c.eps and fused_triplet_step_available(state) and not ops.triplet_direct_mode()
            state, loss = train_step(state, *ids, c.lam, c.batch_size)
            assert len(state.versions) == 2
            state.consolidate()
            assert state.raw_params["params"]["scene_tower"]["embedding"].data_ptr() == v["scene"].data_ptr()
        else:
            assert ops.triplet_direct_mode()
            loss = ops.triplet_train_step(v["scene"], None, None, v["scene_acc"], v["product"], None, None,
                                          v["product_acc"], *ids, c.lam, c.batch_size, c.lr, c.eps, **kw)
        torch.cuda.synchronize()
        return float(loss)


def _check(ref, tables, loss, mode, before=None):
    """rows nobody names and the sentinels keep their bits; everything else within the bounds of the helper"""
    case, after, before = ref.case, tables.raw(), before or tables.before
    for k in R.ARRAYS:
        keep = np.ones(after[k].shape[0], bool)
        keep[PAD:-PAD] = ~ref.touched["scene" if k.startswith("scene") else "product"]
        assert np.array_equal(after[k][keep], before[k][keep]), "%s: a row no id names, or a sentinel row, changed" % k
    got = Tables.values(after)
    if case.dtype == "bf16":
        for k in ("scene", "product"):
            got[k] = after[k][PAD:-PAD].astype(np.uint16)
    ratios, fails = R.compare(ref, got, loss)
    print("%s %s/%s: error / bound %s" % (mode, case.spec.name, case.dtype, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    worst = _WORST.setdefault("%s/%s" % (mode, case.dtype), {})
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)
    assert not fails, fails
    return after


def _one_step(dev, monkeypatch, name, dtype, mode, **kw):
    ref = _reference(name, dtype)
    tables = Tables(ref.case, dev)
    loss = tables.step(mode, monkeypatch, **kw)
    return _check(ref, tables, loss, mode), loss


# ---- widths: one D per (VEC, NCH) instantiation and lane count, B = 384, runs of 1 to 3 --------------------------------
@pytest.mark.parametrize("mode", ["direct", "few", "stamped"])
@pytest.mark.parametrize("D", R.WIDTHS)
def test_widths_f32(dev, monkeypatch, D, mode):
    _one_step(dev, monkeypatch, "width-D%d" % D, "f32", mode)


@pytest.mark.parametrize("D", R.WIDTHS)
def test_widths_bf16(dev, monkeypatch, D):
    _one_step(dev, monkeypatch, "width-D%d" % D, "bf16", "direct")


@pytest.mark.parametrize("D", R.WIDTHS_VEC8)
def test_widths_bf16_vec8(dev, monkeypatch, D):
    """ESR_BF16_VEC8=1: 8-element chunks where D % 8 == 0; D = 12 falls back to 4-element chunks (only the result is
    checked)"""
    _one_step(dev, monkeypatch, "width-D%d" % D, "bf16", "vec8")


# ---- run lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mode", [("f32", "direct"), ("bf16", "direct"), ("f32", "stamped")])
@pytest.mark.parametrize("D", R.RUN_WIDTHS)
@pytest.mark.parametrize("case", R.RUN_CASES)
def test_run_lengths(dev, monkeypatch, case, D, dtype, mode):
    _one_step(dev, monkeypatch, "%s-D%d" % (case, D), dtype, mode)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", R.RUN_WIDTHS)
@pytest.mark.parametrize("k", [8, 9])
def test_runs_of_8_and_9_through_a_plan_and_its_hint(dev, monkeypatch, k, D, dtype):
    """Every run exactly 8 long: the plan's hint stays clear and the step runs with long_runs = 0 (no long-run launch);
    every run exactly 9 long: the hint carries the generation.  Bit for bit the step that plans in line and screens for
    long runs itself (long_runs = -1), and within the bounds of the oracle."""
    from esrecsys_amd import ops
    name = "all%d-D%d" % (k, D)
    plain, loss_plain = _one_step(dev, monkeypatch, name, dtype, "direct", long_runs=-1)
    ref = _reference(name, dtype)
    c = ref.case
    ids = [torch.from_numpy(x).to(dev) for x in (c.sid, c.pid, c.nid)]
    _set_mode(monkeypatch, "direct")
    srt, prm = ops.segment_sort_multi(ids, [0, c.Vs, c.Vs], c.Vs + c.Vp)
    hints = torch.zeros(1, dtype=torch.int32, device=dev)
    plans = ops.triplet_plan([tuple(ids)], c.Vs, srt, prm, hints=hints, gen=7)
    assert int(hints[0]) == (7 if k == 9 else 0)
    tables = Tables(c, dev)
    loss = tables.step("direct", monkeypatch, presorted=(srt, prm), plan=plans[0], long_runs=1 if k == 9 else 0)
    planned = _check(ref, tables, loss, "direct")
    assert loss == loss_plain and all(np.array_equal(planned[a], plain[a]) for a in R.ARRAYS)


# ---- grid-stride: 4096 workgroups of eight triplets, more than any resident count ---------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_grid_stride(dev, monkeypatch, dtype):
    _one_step(dev, monkeypatch, "gridstride-D128", dtype, "direct")


# ---- a second step on the same towers, plan buffer and workspace -------------------------------------------------------
@pytest.mark.parametrize("plan", ["shared", "inline"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_second_step_on_a_used_plan_buffer(dev, monkeypatch, dtype, plan):
    """A batch whose runs are all long (9), then one without a long run (8), on the same towers: what the first step left
    in the side buffer, the run counters, the parked flag and the long-run list must not reach the second.  The second
    reference starts from what the device holds after the first step."""
    import ctypes
    from esrecsys_amd import _lib, ops
    ref_a = _reference("twostep-a-D128", dtype)
    case_b = R.make_second_step(ref_a, "twostep-b-D128")  # ids whose conditions hold on the fp64 state after step one
    tables = Tables(ref_a.case, dev)
    B, Vs, Vp = ref_a.case.B, ref_a.case.Vs, ref_a.case.Vp
    buf = ops._aligned_bytes(ops._ws_bytes("esr_triplet_plan_bytes", B), dev)

    def kw(case, gen):
        if plan == "inline":
            return {}
        _set_mode(monkeypatch, "direct")
        ids = [torch.from_numpy(x).to(dev) for x in (case.sid, case.pid, case.nid)]
        srt, prm = ops.segment_sort_multi(ids, [0, Vs, Vs], Vs + Vp)
        ptrs = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ids])
        _lib.check(_lib.load().esr_triplet_plan(ptrs, 1, B, Vs, srt.data_ptr(), prm.data_ptr(), buf.data_ptr(), None, gen,
                                                ops._stream()), "esr_triplet_plan")
        torch.cuda.synchronize()  # (ids stay alive until the plan has been made)
        return {"presorted": (srt, prm), "plan": buf, "long_runs": -1}
    loss = tables.step("direct", monkeypatch, **kw(ref_a.case, 1))
    mid = _check(ref_a, tables, loss, "direct")
    case_b = R.with_inputs(case_b, *(Tables.values(mid)[k] for k in R.ARRAYS))
    m, g, _ = R.input_conditions(case_b)
    assert m >= R.MIN_MARGIN and g >= R.MIN_NORM_GAP
    ref_b = case_b.reference()
    tables.case = case_b
    loss = tables.step("direct", monkeypatch, **kw(case_b, 2))
    _check(ref_b, tables, loss, "direct", before=mid)


# ---- the argument check -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [253, 254])
def test_widest_scalar_rows_the_argument_check_lets_in(dev, monkeypatch, D):
    """(D = 255 and D = 1024, the limits themselves, are among the widths above)"""
    _one_step(dev, monkeypatch, "edge-D%d" % D, "f32", "direct")


def _plain_case(D, dtype, B=8, V=16):
    spec = R.Spec("refused-D%d" % D, D, B, Vs=V, Vp=V)
    rng = np.random.default_rng(D)
    t = [R.o_optim.round_bf16((rng.standard_normal((V, D)) * 0.3).astype(np.float32)) for _ in range(2)]
    ids = [rng.integers(0, V, B).astype(np.int32) for _ in range(3)]
    return R.Case(spec, dtype, 0, t[0], t[1], np.full_like(t[0], 0.1), np.full_like(t[1], 0.1), *ids)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", [257, 258, 259, 1028])
def test_rows_too_wide_are_refused_and_nothing_is_written(dev, monkeypatch, D, dtype):
    """more than four chunks per lane: scalar rows beyond 256 elements, float4 rows beyond 1024"""
    from esrecsys_amd._lib import EsrLibraryError
    tables = Tables(_plain_case(D, dtype), dev)
    for mode in ("direct", "few") + (("stamped",) if dtype == "f32" else ("vec8",)):
        with pytest.raises(EsrLibraryError, match=r"esr_triplet_train_step: D=%d not supported" % D):
            tables.step(mode, monkeypatch)
    after = tables.raw()
    assert all(np.array_equal(after[k], tables.before[k]) for k in R.ARRAYS)


def test_other_refusals_leave_the_tables_alone(dev, monkeypatch):
    from esrecsys_amd import ops
    from esrecsys_amd._lib import EsrLibraryError
    tables = Tables(_plain_case(12, "bf16"), dev)
    c, v = tables.case, tables.views
    ids = [torch.from_numpy(x).to(dev) for x in (c.sid, c.pid, c.nid)]
    _set_mode(monkeypatch, "stamped")
    with pytest.raises(TypeError, match=r"bf16 towers need the direct step \(ESR_TRIPLET_STEP=stamped is set\)"):
        ops.triplet_train_step(v["scene"], None, None, v["scene_acc"], v["product"], None, None, v["product_acc"], *ids, 0.1,
                               8.0, 0.05)
    tables.case.batch_size = 0.0
    with pytest.raises(EsrLibraryError, match="esr_triplet_train_step: batch_size must be non-zero"):
        tables.step("direct", monkeypatch)
    # a bf16 tower of float4-wide rows that is not 8-byte aligned
    flat = torch.zeros(c.Vs * c.D + 4, dtype=torch.bfloat16, device=dev)
    odd = flat[1:1 + c.Vs * c.D].view(c.Vs, c.D)
    assert odd.data_ptr() % 8 == 2 and odd.is_contiguous()
    _set_mode(monkeypatch, "direct")
    with pytest.raises(EsrLibraryError, match="esr_triplet_train_step: bf16 tables must be 8-byte aligned"):
        ops.triplet_train_step(odd, None, None, v["scene_acc"], v["product"], None, None, v["product_acc"], *ids, 0.1, 8.0,
                               0.05)
    torch.cuda.synchronize()
    after = tables.raw()
    assert all(np.array_equal(after[k], tables.before[k]) for k in R.ARRAYS) and not bool(flat.any())

"""GPU: ONE step of the one-pass GloVe train step (esr_glove.hip: esr_glove_train_step, esr_glove_train_steps,
esr_glove_plan) against the fp64 oracle (tests/_glove_step_ref.py: oracle.glove.loss_and_grads + row_grads +
oracle.optim.sparse_adagrad_update), on every path the unit dispatches: every (VEC, NCH) instantiation and lane count in
both loss modes, f32 and bf16 embedding tables, ESR_BF16_VEC8=1 with its two fallbacks, runs of 1 .. 97 with their chunk
edges, lists around kFinFuseMaxIds and kResolveMinIds, grids beyond the resident count, the statistics workgroups' edges,
plans made ahead against plans made in line with every long_runs value, a second step on a used workspace and plan
buffer, a group of three steps by one library call, and the argument refusals.

ops.glove_train_step is called on hand-made tables: every array is a view between 64 sentinel rows of NaN bits (the
location bytes between 64 bytes 0xEE), every row starts with a random stamped location byte, its live value in the buffer
bit 0 names and NaN bits in its dead copy.  Exact in every case: the sentinels, both copies and the byte of a row no id
names, the copy a touched row was read from; a touched row's byte has bit 0 flipped and carries the step's stamp.  The
values, read from the buffer a row had to move to: kernel error against fp64 <= 4 e32 + 2^-22 per table and per touched
row, e32 = the same oracle in float32 (the loss: relative); a bf16 embedding is bit-equal to round_bf16(fp64 result)
except where the fp64 value is within the row's bound of a tie (the helper's docstring has the exact form).  Input
conditions (targets on both sides of the clip, every occurrence's own term of its row's update >= 64 x the row's bound
for 99 % of them, < 1 % of the touched elements near a bf16 tie) are asserted on the fp64 reference by the helper's
make_case before any GPU work.

Largest error / bound seen per mode and table type on an MI355X (printed at the end of a run with -s; "/row" = the
largest over the touched rows, each against its own bound; a bf16 embedding has no ratio, it is compared bit for bit):
    reference f32   loss 0.343  emb 0.296 /row 0.378  emb_acc 0.340 /row 0.503  bias 0.224 /row 0.232  bias_acc 0.364 /row 0.740
    diagonal  f32   loss 0.333  emb 0.239 /row 0.332  emb_acc 0.424 /row 0.617  bias 0.306 /row 0.574  bias_acc 0.372 /row 0.673
    reference bf16  loss 0.351                        emb_acc 0.413 /row 0.863  bias 0.152 /row 0.256  bias_acc 0.438 /row 0.788
    diagonal  bf16  loss 0.345                        emb_acc 0.344 /row 0.688  bias 0.242 /row 0.357  bias_acc 0.179 /row 0.494
No mode needs the whole bound, so no class of cases needed an f32 oracle summed in the kernel's order: with runs of at most
97 the step's arithmetic (A - sbar C in reference mode, fp64 bias runs) is an f32 evaluation of the oracle's on every path.
"""
import ctypes

import numpy as np
import pytest
import torch

import _glove_step_ref as R

pytestmark = pytest.mark.gpu

PAD = 64          # sentinel rows in front of and behind every array
LOC_SENTINEL = 0xEE
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    for key in sorted(_WORST):
        print("\nlargest error / (4 e32 + 2^-22), %s: %s" % (key, ", ".join("%s %.3f" % kv for kv in sorted(_WORST[key].items()))))


def _env(monkeypatch, vec8=False):
    for var in ("ESR_BF16_VEC8", "ESR_GLOVE_FIN_FUSED", "ESR_GLOVE_FUSED"):
        monkeypatch.delenv(var, raising=False)
    if vec8:
        monkeypatch.setenv("ESR_BF16_VEC8", "1")


def _mode_const(mode):
    from esrecsys_amd import ops
    return {"reference": ops.GLOVE_REFERENCE, "diagonal": ops.GLOVE_DIAGONAL}[mode]


def _dev_batch(case, dev):
    return (torch.from_numpy(np.ascontiguousarray(case.inputs, np.int32)).to(dev),
            torch.from_numpy(np.ascontiguousarray(case.target, np.float32)).to(dev))


class Tables:
    """the six arrays of a case on the device, as raw integers: each a [V, ...] view between PAD sentinel rows of a larger
    buffer; `shift` = elements by which the two embedding buffers are moved off their 16-byte alignment"""
    NAMES = ("emb0", "emb1", "loc", "emb_acc", "bias", "bias_acc")

    def __init__(self, V, D, dtype, dev, shift=0):
        self.V, self.D, self.bf16, self.dev = V, D, dtype == "bf16", dev
        rows = V + 2 * PAD
        self.flat, self.bufs = {}, {}
        for k in self.NAMES:
            emb = k in ("emb0", "emb1")
            width = D if k in ("emb0", "emb1", "emb_acc") else 1
            idt = torch.uint8 if k == "loc" else torch.int16 if (emb and self.bf16) else torch.int32
            off = shift if emb else 0
            flat = torch.empty(rows * width + 8, dtype=idt, device=dev)
            flat.fill_(LOC_SENTINEL if k == "loc" else _signed(R.NAN16, 16) if idt == torch.int16 else _signed(R.NAN32, 32))
            self.flat[k] = flat
            self.bufs[k] = flat[off:off + rows * width].view(rows, width)
        self.fresh = {k: f.cpu().numpy() for k, f in self.flat.items()}

    def table(self, k):
        """the [V, D] / [V] tensor handed to the library"""
        v = self.bufs[k][PAD:PAD + self.V]
        if k == "loc":
            return v.view(self.V)
        if k in ("emb0", "emb1"):
            v = v.view(torch.bfloat16 if self.bf16 else torch.float32)
        else:
            v = v.view(torch.float32)
        return v if k in ("emb0", "emb1", "emb_acc") else v.view(self.V)

    def load(self, state):
        for k, a in zip(self.NAMES, (state.emb[0], state.emb[1], state.loc, state.emb_acc, state.bias, state.bias_acc)):
            a = np.ascontiguousarray(a)
            a = a if a.dtype == np.uint8 else a.view(np.int16 if a.dtype == np.uint16 else np.int32)
            self.bufs[k][PAD:PAD + self.V].copy_(torch.from_numpy(a.reshape(self.V, -1)).to(self.dev))
        got = self.state()
        assert all(np.array_equal(a, b) for a, b in zip(_parts(got), _parts(state)))  # the upload was exact
        return got

    def state(self):
        """R.State of the views, after checking that every sentinel (and the slack around a shifted buffer) is intact"""
        torch.cuda.synchronize()
        out = {}
        for k, f in self.flat.items():
            a = f.cpu().numpy()
            off = self.bufs[k].data_ptr() - f.data_ptr()
            lo = off // a.itemsize + PAD * self.bufs[k].shape[1]
            hi = lo + self.V * self.bufs[k].shape[1]
            assert np.array_equal(a[:lo], self.fresh[k][:lo]) and np.array_equal(a[hi:], self.fresh[k][hi:]), \
                "%s: a sentinel in front of or behind the table changed" % k
            v = a[lo:hi]
            out[k] = v if k == "loc" else v.view(np.uint16 if v.dtype == np.int16 else np.uint32)
        D = self.D
        return R.State(out["emb0"].reshape(-1, D), out["emb1"].reshape(-1, D), out["loc"], out["emb_acc"].reshape(-1, D),
                       out["bias"], out["bias_acc"])

    def args(self):
        return tuple(self.table(k) for k in self.NAMES)

    def step(self, case, batch=None, **kw):
        """one step through ops.glove_train_step; returns the loss"""
        from esrecsys_amd import ops
        inputs, target = batch or _dev_batch(case, self.dev)
        loss = ops.glove_train_step(*self.args(), inputs, target, _mode_const(case.mode), case.lr, case.eps,
                                    stamp=case.stamp, **kw)
        torch.cuda.synchronize()
        return float(loss)


def _signed(bits, width):
    return bits - (1 << width) if bits >> (width - 1) else bits


def _parts(state):
    return (state.emb[0], state.emb[1], state.loc, state.emb_acc, state.bias, state.bias_acc)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_parts(a), _parts(b)))


def _check(ref, before, after, loss, tag):
    case = ref.case
    ratios, fails = R.compare(ref, before, after, loss)
    print("%s %s/%s/%s: error / bound %s" % (tag, case.spec.name, case.dtype, case.mode,
                                             ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    worst = _WORST.setdefault("%s/%s" % (case.mode, case.dtype), {})
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)
    assert not fails, fails


def _one_step(dev, monkeypatch, name, dtype, mode, vec8=False, shift=0, tag="inline", **kw):
    case = R.make_case(name, dtype, mode)  # (asserts the input conditions)
    ref = case.reference()
    tables = Tables(case.V, case.D, dtype, dev, shift)
    before = tables.load(R.initial_state(case))
    _env(monkeypatch, vec8)
    loss = tables.step(case, **kw)
    after = tables.state()
    _check(ref, before, after, loss, "vec8" if vec8 else tag)
    return after, loss


def _plan(case, dev, gen=7):
    """(batch, presorted, plan, hint) of a plan made ahead: ops.segment_sort + ops.glove_plan"""
    from esrecsys_amd import ops
    batch = _dev_batch(case, dev)
    srt, prm = ops.segment_sort(batch[0].reshape(-1), case.V)
    hints = torch.zeros(1, dtype=torch.int32, device=dev)
    plans = ops.glove_plan([batch[0]], [batch[1]], srt, prm, hints=hints, gen=gen)
    assert np.array_equal(srt.cpu().numpy(), R.sorted_ids(case.inputs))
    return batch, (srt, prm), plans[0], int(hints[0])


# ---- widths: one D per (VEC, NCH) instantiation and lane count, B = 384, runs of 1 to 3 --------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_widths_f32(dev, monkeypatch, D, mode):
    _one_step(dev, monkeypatch, "width-D%d" % D, "f32", mode)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("D", R.WIDTHS)
def test_widths_bf16(dev, monkeypatch, D, mode):
    _one_step(dev, monkeypatch, "width-D%d" % D, "bf16", mode)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("D", R.WIDTHS_VEC8)
def test_widths_bf16_vec8(dev, monkeypatch, D, mode):
    """ESR_BF16_VEC8=1: 8-element chunks where D % 8 == 0; D = 12 falls back to 4-element chunks"""
    _one_step(dev, monkeypatch, "width-D%d" % D, "bf16", mode, vec8=True)


@pytest.mark.parametrize("D", [128, 520])
def test_bf16_vec8_falls_back_on_a_table_that_is_only_8_byte_aligned(dev, monkeypatch, D):
    """both buffers 8 bytes off a 16-byte boundary: ESR_BF16_VEC8=1 must take the 4-element path -- the same bits as
    without the variable on an aligned table"""
    name = "width-D%d" % D
    plain, loss_plain = _one_step(dev, monkeypatch, name, "bf16", "reference")
    tables = Tables(R.SPECS[name].V, D, "bf16", dev, shift=4)
    assert all(tables.table(k).data_ptr() % 16 == 8 for k in ("emb0", "emb1"))
    moved, loss = _one_step(dev, monkeypatch, name, "bf16", "reference", vec8=True, shift=4)
    assert loss == loss_plain and _same_bits(moved, plain)


# ---- run lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", R.RUN_WIDTHS)
@pytest.mark.parametrize("case", R.RUN_CASES)
def test_run_lengths(dev, monkeypatch, case, D, dtype, mode):
    _one_step(dev, monkeypatch, "%s-D%d" % (case, D), dtype, mode)


# ---- thresholds of the dispatch ----------------------------------------------------------------------------------------
_THRESHOLDS = [(n, "f32", m) for n in R.THRESHOLD_CASES for m in (R.MODES if R.SPECS[n].D == 8 else R.MODES[:1])] + \
              [(n, "bf16", "reference") for n in R.RESOLVED_CASES]


@pytest.mark.parametrize("planned", [False, True])
@pytest.mark.parametrize("name,dtype,mode", _THRESHOLDS)
def test_thresholds(dev, monkeypatch, name, dtype, mode, planned):
    """lists around kFinFuseMaxIds (planned, long_runs = 0: the update kernel's last workgroup is the finalize step up to
    8192 ids) and kResolveMinIds, grids beyond the resident count, one and two statistics workgroups; each with the plan
    made in line and made ahead (the resolved path ignores the plan and takes long_runs as the caller's word)"""
    if not planned:
        _one_step(dev, monkeypatch, name, dtype, mode)
        return
    _env(monkeypatch)
    case = R.make_case(name, dtype, mode)
    batch, presorted, plan, hint = _plan(case, dev)
    assert hint == 0  # runs of 1 to 3
    _one_step(dev, monkeypatch, name, dtype, mode, tag="planned", batch=batch, presorted=presorted, plan=plan, long_runs=0)


# ---- a plan made ahead and its hint, against the plan made in line ------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["ladder-D128", "run33-a0-D128", "ladder-D6", "run33-a0-D6"])
def test_planned_step_equals_in_line_step(dev, monkeypatch, name, dtype, mode):
    """No run over 32: the hint stays clear and the step may run with long_runs = 0 (no long-run launch, finalize inside
    the update kernel); a run of 33: the hint carries the generation.  With the plan and the hint's long_runs, and with
    long_runs = -1: bit for bit the in-line step, and within the oracle's bounds."""
    plain, loss_plain = _one_step(dev, monkeypatch, name, dtype, mode)
    case = R.make_case(name, dtype, mode)
    long_run = name.startswith("run33")
    batch, presorted, plan, hint = _plan(case, dev, gen=7)
    assert hint == (7 if long_run else 0)
    for long_runs in (1 if long_run else 0, -1):
        batch, presorted, plan, _ = _plan(case, dev)  # (a plan record feeds exactly one step)
        got, loss = _one_step(dev, monkeypatch, name, dtype, mode, tag="planned", batch=batch, presorted=presorted,
                              plan=plan, long_runs=long_runs)
        assert loss == loss_plain and _same_bits(got, plain), long_runs
    # sorted ahead, planned in line
    got, loss = _one_step(dev, monkeypatch, name, dtype, mode, tag="presorted", batch=batch, presorted=presorted)
    assert loss == loss_plain and _same_bits(got, plain)


# ---- through the library: own workspace and plan buffer ------------------------------------------------------------------
class LibStep:
    """esr_glove_train_step / esr_glove_plan / esr_glove_train_steps called as train_cooccurence.py calls them, on ONE
    workspace and ONE plan buffer that stay"""

    def __init__(self, tables, B, nplans=1):
        from esrecsys_amd import _lib, ops
        self.lib, self.check, self.ops, self.tables, self.B = _lib.load(), _lib.check, ops, tables, B
        self.ws = ops._ws(ops._ws_bytes("esr_glove_step_workspace_bytes", B, tables.D), tables.dev)
        self.pbytes = ops._ws_bytes("esr_glove_plan_bytes", B)
        self.plans = ops._aligned_bytes(nplans * self.pbytes, tables.dev)
        t = tables.args()
        self.fixed = tuple(x.data_ptr() for x in t) + (tables.V, ops._table_dtype(t[0], "emb"), tables.D)

    def sort_and_plan(self, batches, gen):
        """sorted ids, perm [nb, 2 B] and the plan records of the batches in self.plans; returns (srt, prm, hints)"""
        nb, dev = len(batches), self.tables.dev
        srt = torch.empty((nb, 2 * self.B), dtype=torch.int32, device=dev)
        prm = torch.empty_like(srt)
        for b, (inputs, _) in enumerate(batches):
            self.ops.segment_sort(inputs.reshape(-1), self.tables.V, out=(srt[b], prm[b]))
        hints = torch.zeros(nb, dtype=torch.int32, device=dev)
        ip = (ctypes.c_void_p * nb)(*[i.data_ptr() for i, _ in batches])
        tp = (ctypes.c_void_p * nb)(*[t.data_ptr() for _, t in batches])
        self.check(self.lib.esr_glove_plan(ip, tp, nb, self.B, srt.data_ptr(), prm.data_ptr(), self.plans.data_ptr(),
                                           hints.data_ptr(), gen, self.ops._stream()), "esr_glove_plan")
        torch.cuda.synchronize()
        return srt, prm, hints.cpu().tolist()

    def step(self, case, batch, presorted=None, planned=False, long_runs=-1, ws_bytes=None):
        loss = torch.empty(1, dtype=torch.float32, device=self.tables.dev)
        srt, prm = presorted if presorted is not None else (None, None)
        self.check(self.lib.esr_glove_train_step(
            *self.fixed, batch[0].data_ptr(), batch[1].data_ptr(), self.B, _mode_const(case.mode), case.lr, case.eps,
            case.stamp, self.ops._p(srt), self.ops._p(prm), self.plans.data_ptr() if planned else None, long_runs, 0, None,
            0, loss.data_ptr(), self.ws.data_ptr(), self.ws.numel() if ws_bytes is None else ws_bytes, self.ops._stream()),
            "esr_glove_train_step")
        torch.cuda.synchronize()
        return float(loss)


@pytest.mark.parametrize("planned", [False, True])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_second_step_on_a_used_workspace_and_plan_buffer(dev, monkeypatch, dtype, mode, planned):
    """A batch with a run of 97 (three partial sums parked, the long-run launch combines them), then one whose longest
    run is 32, on the same tables, workspace and plan buffer, stamps 126 and 127: the statistics, loss and flag words and
    the parked partials of the first step must not reach the second.  The second reference starts from what the device
    holds after the first step (dead copies poisoned again)."""
    _env(monkeypatch)
    a = R.make_case("run97-a31-D128", dtype, mode)
    a = R.with_state(a, a.arrays(), R.draw_loc(np.random.default_rng(126), a.V, 126, 127), stamp=126)
    tables = Tables(a.V, a.D, dtype, dev)
    lib = LibStep(tables, a.B)

    def run(case, gen, want_hint):
        before = tables.load(R.initial_state(case))
        batch = _dev_batch(case, dev)
        kw = {}
        if planned:
            srt, prm, hints = lib.sort_and_plan([batch], gen)
            assert hints == [want_hint]
            kw = {"presorted": (srt[0], prm[0]), "planned": True, "long_runs": 1 if want_hint else 0}
        loss = lib.step(case, batch, **kw)
        after = tables.state()
        _check(case.reference(), before, after, loss, "lib-planned" if planned else "lib-inline")
        return after
    assert R.conditions_hold(R.input_conditions(a))
    mid = run(a, 3, 3)
    b = R.next_case(a, "ladder-D128")                  # ids whose conditions hold on the fp64 state after step one ...
    b = R.with_state(b, mid.live(), mid.loc.copy())    # ... on what the device holds
    assert b.stamp == 127 and R.conditions_hold(R.input_conditions(b))
    run(b, 4, 0)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_group_of_three_steps_by_one_library_call(dev, monkeypatch, dtype, mode):
    """esr_glove_train_steps on three planned batches (a run of 65, all runs 1, runs of 2 .. 32), stamps 125 .. 127, with
    the hints' long_runs and with none given: bit for bit three single in-line steps with the same stamps; the last
    state against the oracle chained over the three steps (f32 tables), every single step against the oracle of one
    step."""
    _env(monkeypatch)
    cases = R.chain_cases(["run65-a0-D128", "ones-D128", "ladder-D128"], dtype, mode, first_stamp=125)
    ref = R.chain_reference(cases)
    first = cases[0]
    tables = Tables(first.V, first.D, dtype, dev)
    start = R.initial_state(first)
    batches = [_dev_batch(c, dev) for c in cases]
    before = tables.load(start)
    single, want = [], before
    for c, b in zip(cases, batches):  # every single step against the oracle that starts from what the device holds
        prev, c = want, R.with_state(c, want.live(), want.loc.copy())
        assert R.conditions_hold(R.input_conditions(c))
        single.append(tables.step(c, batch=b))
        want = tables.state()
        _check(c.reference(), prev, want, single[-1], "single")
    lib = LibStep(tables, first.B, nplans=3)
    for given in (True, False):
        tables.load(start)
        srt, prm, hints = lib.sort_and_plan(batches, 9)
        assert hints == [9, 0, 0]
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        ip = (ctypes.c_void_p * 3)(*[i.data_ptr() for i, _ in batches])
        tp = (ctypes.c_void_p * 3)(*[t.data_ptr() for _, t in batches])
        long_runs = (ctypes.c_int32 * 3)(1, 0, 0) if given else None
        lib.check(lib.lib.esr_glove_train_steps(*lib.fixed, 3, ip, tp, first.B, _mode_const(mode), first.lr, first.eps, 125,
                                                srt.data_ptr(), prm.data_ptr(), lib.plans.data_ptr(), long_runs,
                                                losses.data_ptr(), lib.ws.data_ptr(), lib.ws.numel(), lib.ops._stream()),
                  "esr_glove_train_steps")
        got = tables.state()
        assert losses.cpu().tolist() == single and _same_bits(got, want), given
    # the chained oracle: bytes, untouched rows, and -- f32 tables -- the live values of the last state.  (A bf16 table may
    # leave a step one ulp from the oracle's at a tie, 2^-8 of the element: the steps after it are then steps on other
    # inputs, so bf16 tables have the three checks above instead.)
    t = ref.touched
    assert np.array_equal(want.loc, R.chain_loc(cases))
    for buf in (0, 1):
        assert np.array_equal(want.emb[buf][~t], before.emb[buf][~t])
    live = want.live()
    raw = np.where((want.loc & 1).astype(bool)[:, None], want.emb[1], want.emb[0])
    got = {"emb": raw if dtype == "bf16" else live[0], "emb_acc": live[1], "bias": live[2], "bias_acc": live[3]}
    ratios, fails = R.compare_values(ref, got, single[2])
    print("three steps %s/%s: error / bound %s" % (dtype, mode, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    assert dtype == "bf16" or not fails, fails


# ---- the argument check -------------------------------------------------------------------------------------------------
def _plain(D, dtype, dev, V=16, B=8, shift=0):
    spec = R.Spec("refused-D%d" % D, D, B, V)
    rng = np.random.default_rng(D)
    emb = R.o_optim.round_bf16((rng.standard_normal((V, D)) * 0.3).astype(np.float32))
    case = R.Case(spec, dtype, "reference", 0, emb, np.full_like(emb, 0.1), np.zeros(V, np.float32),
                  np.full(V, 0.1, np.float32), R.draw_loc(rng, V, R.STAMP), rng.integers(0, V, (2, B)).astype(np.int32),
                  rng.uniform(1.0, 300.0, B).astype(np.float32))
    tables = Tables(V, D, dtype, dev, shift)
    return case, tables, tables.load(R.initial_state(case))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("D", R.REFUSED_WIDTHS)
def test_rows_too_wide_are_refused_and_nothing_is_written(dev, monkeypatch, D, dtype):
    """more than four chunks per lane: scalar rows beyond 256 elements, float4 rows beyond 1024"""
    from esrecsys_amd._lib import EsrLibraryError
    case, tables, before = _plain(D, dtype, dev)
    for vec8 in (False, True):
        _env(monkeypatch, vec8)
        with pytest.raises(EsrLibraryError, match=r"esr_glove_train_step: D=%d not supported" % D):
            tables.step(case)
    assert _same_bits(tables.state(), before)


def test_other_refusals_leave_the_tables_alone(dev, monkeypatch):
    from esrecsys_amd import ops
    from esrecsys_amd._lib import EsrLibraryError
    _env(monkeypatch)
    case, tables, before = _plain(12, "bf16", dev)
    batch = _dev_batch(case, dev)
    emb0, emb1, loc, acc, bias, bias_acc = tables.args()
    step = lambda *t, **kw: ops.glove_train_step(*t, *batch, ops.GLOVE_REFERENCE, case.lr, case.eps, **kw)  # noqa: E731
    with pytest.raises(EsrLibraryError, match="esr_glove_train_step: the shadow table must be a second buffer"):
        step(emb0, emb0, loc, acc, bias, bias_acc, stamp=5)
    for stamp in (0, 128):
        with pytest.raises(EsrLibraryError, match=r"esr_glove_train_step: stamp %d not in \[1, 127\]" % stamp):
            step(*tables.args(), stamp=stamp)
    with pytest.raises(ValueError, match="needs the step's stamp"):
        step(*tables.args())
    with pytest.raises(EsrLibraryError, match="esr_glove_train_step: bad mode 7"):
        ops.glove_train_step(*tables.args(), *batch, 7, case.lr, case.eps, stamp=5)
    _, _, plan, _ = _plan(case, dev)
    with pytest.raises(EsrLibraryError, match="esr_glove_train_step: a plan goes with the sorted ids it was made from"):
        step(*tables.args(), stamp=5, plan=plan)
    lib = LibStep(tables, case.B)
    with pytest.raises(EsrLibraryError, match=r"esr_glove_train_step: workspace \d+ bytes < \d+ required"):
        lib.step(case, batch, ws_bytes=lib.ws.numel() - 256)
    assert _same_bits(tables.state(), before)
    # a bf16 table of float4-wide rows that is not 8-byte aligned (one element off), as either buffer
    case, odd, before = _plain(12, "bf16", dev, shift=1)
    assert odd.table("emb0").data_ptr() % 8 == 2
    for t in ((odd.table("emb0"), emb1), (emb0, odd.table("emb1"))):
        with pytest.raises(EsrLibraryError, match="esr_glove_train_step: bf16 tables must be 8-byte aligned"):
            step(*t, loc, acc, bias, bias_acc, stamp=5)
    torch.cuda.synchronize()
    assert _same_bits(odd.state(), before)
    # ... while scalar-wide rows (D % 4 != 0) need no alignment: a step on tables one element off runs and is right
    _one_step(dev, monkeypatch, "width-D6", "bf16", "reference", shift=1, tag="odd")

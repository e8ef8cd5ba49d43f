"""GPU: ONE step of the one-call in-batch train step (ops.inbatch_train_step -> esr_inbatch_train_step_f16x2) against the
fp64 oracle (tests/_inbatch_step_ref.py: oracle.stl_head.inbatch_softmax_loss_and_grads + oracle.optim.
sparse_adagrad_update), per element, on every path the call dispatches: f32 towers (two fp16 planes) and bf16 towers (the
one-plane kernels), every batch size with its own pass-Q split count, every width class of the zero-padded tile, and the
update tail in each of its forms --

    sort            presorted=None: the sort inside the call, then merge + range update
    presorted       the list from ops.segment_sort_batched, long_runs=-1: merge + update with the long-run launch
    hint0           presorted, long_runs=0: the merging update at D = 128, merge + update with skip_long below
    hint0-nomerge   as hint0 with ESR_IB2H_MERGE_UPDATE=0: merge + update
    side, side0     side_stream given, long_runs=-1 / 0: f32 towers take the overlapped form (the query tower's update
                    beside pass C, both merges read the row copies), bf16 towers ignore the stream
    state           train_step on a TrainState with neg=None: the drop-in path

-- over id lists whose sorted occurrence list has runs of every class at every alignment the update distinguishes (see
the helper's geometry_specs).  Only cases whose longest run is <= 32 run with long_runs=0; the hint comes from
ops.long_run_hint and is held to the helper's own answer.

Bounds (worked out per case, see the helper): kernel error against fp64 <= 4 e32 + 2^-22 for both towers, both
accumulators, lse and the loss, e32 = the same oracle in float32.  bf16 towers: bit-equal to round_bf16(fp64 result)
except one bf16 ulp where the fp64 value is within that distance of a tie.  Exact in every case: rows no id names, and 64
sentinel rows of NaN bits in front of and behind every table and accumulator, keep their bits; the uploads are exact; and
all modes of one case leave the same bits in loss, lse, towers and accumulators.  Input conditions (every | |row| - 1 | >=
1e-3, both sides of the kink, the runs where the spec puts them, a finite reference) are asserted by the helper's
make_case before any GPU work.

Largest error / bound seen per mode on an MI355X (printed at the end of a run with -s; bf16 towers have no ratio, they
are compared bit for bit):
    sort, presorted, side   f32   loss 0.255  lse 0.301  query 0.145  cand 0.150  query_acc 0.334  cand_acc 0.139
    state                   f32   loss 0.255             query 0.145  cand 0.150  query_acc 0.334  cand_acc 0.139
    hint0, hint0-nomerge,
    side0                   f32   loss 0.250  lse 0.301  query 0.111  cand 0.125  query_acc 0.118  cand_acc 0.134
    every mode              bf16  loss 0.265  lse 0.292                           query_acc 0.124  cand_acc 0.470
(state hands out no lse; the hinted modes leave out the cases with a run longer than 32, which hold the largest
accumulator ratio.)  No mode needs half of the bound: on every path the step is an f32-grade evaluation of the oracle, the
error of the fp16 x 2 products (about 3 * 2^-24 |a||b|) included, so the bound carries no extra term for them.
"""
import numpy as np
import pytest
import torch

import _inbatch_step_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                     # sentinel rows in front of and behind every table
NAN32, NAN16 = 0x7FC0BEEF, 0x7FC1
MODES = ("sort", "presorted", "hint0", "hint0-nomerge", "side", "side0", "state")
HINTED = ("hint0", "hint0-nomerge", "side0")   # long_runs=0: only for cases without a run longer than a chunk
_ENV = ("ESR_IB2H_MERGE_UPDATE", "ESR_IB2H_REF", "ESR_IB2H_FUSED", "ESR_IB2H_BF16", "ESR_IB2H_PC", "ESR_IB2H_POLL",
        "ESR_IB2H_Q_PER_CU", "ESR_INBATCH_AUTO", "ESR_INBATCH_BF16_TABLES")
_WORST = {}
_BITS = {}                   # (case, dtype) -> (mode, loss, lse, raw tables) of the first mode that ran it


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    _BITS.clear()
    for key in sorted(_WORST):
        print("\nlargest error / (4 e32 + 2^-22), %s: %s" % (key, ", ".join("%s %.3f" % kv for kv in sorted(_WORST[key].items()))))


def _set_mode(monkeypatch, mode):
    for var in _ENV:
        monkeypatch.delenv(var, raising=False)
    if mode == "hint0-nomerge":
        monkeypatch.setenv("ESR_IB2H_MERGE_UPDATE", "0")


def _reference(name, dtype):
    """fp64 / f32 oracle of a case, computed once for every mode that runs it (the input conditions are asserted by
    make_case, before any GPU work)"""
    return R.make_case(name, dtype).reference()


class Tables:
    """the four arrays of a case on the device, each a [V, D] view between PAD sentinel rows of a larger buffer"""

    def __init__(self, case, dev):
        self.case, self.bufs, self.views = case, {}, {}
        for k, a in zip(R.ARRAYS, case.inputs()):
            bf16 = case.dtype == "bf16" and k in R.TOWERS
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
            assert a.dtype == np.float32 and np.array_equal(self.values(self.before)[k], a)

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

    def step(self, mode, monkeypatch):
        """one step in `mode`; returns (loss, lse or None) as NumPy f32"""
        from esrecsys_amd import ops
        c, v, dev = self.case, self.views, self.views["query"].device
        qi, ci = (torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(dev) for x in (c.qid, c.cid))
        _set_mode(monkeypatch, mode)
        assert mode not in HINTED or not R.has_long_run(c)
        if mode == "state":
            import esrecsys_amd.pinterest.train_shop_the_look as stl
            from esrecsys_amd import TrainState, optim
            monkeypatch.setattr(stl, "_INBATCH_ONECALL", True)
            monkeypatch.setattr(stl, "_INBATCH_OVERLAP", False)
            tree = lambda s, p: {"params": {"scene_tower": {"embedding": s}, "product_tower": {"embedding": p}}}  # noqa: E731
            state = TrainState(step=0, apply_fn=None, params=tree(v["query"], v["cand"]),
                               tx=optim.sparse_adagrad(c.lr, eps=c.eps),
                               opt_state={"sum_of_squares": tree(v["query_acc"], v["cand_acc"])})
            assert stl._inbatch_one_call(state, v["query"], v["cand"], c.B, "f16x2")
            state, loss = stl.train_step(state, qi, ci, None, c.lam, c.batch_size, scale=c.scale, precision="f16x2")
            assert int(state.step) == 1 and stl._tables(state)[1].data_ptr() == v["query"].data_ptr()
            lse = None
        else:
            kw = {}
            if mode != "sort":
                srt, prm = ops.segment_sort_batched([[qi, ci]], (0, c.Vq), c.Vq + c.Vc)
                assert np.array_equal(srt[0].cpu().numpy(), R.sorted_occurrences(c)[0])
                hint = torch.zeros(1, dtype=torch.int32, device=dev)
                ops.long_run_hint(srt[0], R.SEG_CHUNK, hint, 5)
                assert int(hint[0]) == (5 if R.has_long_run(c) else 0)
                kw = {"presorted": (srt[0], prm[0]), "long_runs": 0 if mode in HINTED else -1}
            if mode in ("side", "side0"):
                kw["side_stream"] = torch.cuda.Stream(device=dev)
            loss, lse = ops.inbatch_train_step(v["query"], v["query_acc"], v["cand"], v["cand_acc"], qi, ci, c.scale, c.lam,
                                               c.batch_size, c.lr, c.eps, want_lse=True, **kw)
        torch.cuda.synchronize()
        return loss.reshape(()).cpu().numpy(), None if lse is None else lse.cpu().numpy()


def _check(ref, tables, loss, lse, mode, before=None):
    """rows nobody names and the sentinels keep their bits; everything else within the bounds of the helper"""
    case, after, before = ref.case, tables.raw(), before or tables.before
    for k in R.ARRAYS:
        keep = np.ones(after[k].shape[0], bool)
        keep[PAD:-PAD] = ~ref.touched["query" if k.startswith("query") else "cand"]
        assert np.array_equal(after[k][keep], before[k][keep]), "%s: a row no id names, or a sentinel row, changed" % k
    got = Tables.values(after)
    if case.dtype == "bf16":
        for k in R.TOWERS:
            got[k] = after[k][PAD:-PAD].astype(np.uint16)
    ratios, fails = R.compare(ref, got, loss, lse)
    print("%s %s/%s: error / bound %s" % (mode, case.spec.name, case.dtype, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    worst = _WORST.setdefault("%s/%s" % (mode, case.dtype), {})
    for k, r in ratios.items():
        worst[k] = max(worst.get(k, 0.0), r)
    assert not fails, fails
    return after


def _one_step(dev, monkeypatch, name, dtype, mode):
    """a step of case `name` in `mode` against the oracle, and bit for bit against the first mode that ran the case"""
    ref = _reference(name, dtype)
    if mode in HINTED and R.has_long_run(ref.case):
        assert name in LONG_CASES  # (the parametrisation leaves these out; a hinted step on them would be the false hint)
        return
    tables = Tables(ref.case, dev)
    loss, lse = tables.step(mode, monkeypatch)
    after = _check(ref, tables, loss, lse, mode)
    first = _BITS.setdefault((name, dtype), (mode, loss, lse, after))
    if first[0] != mode:
        assert loss.tobytes() == first[1].tobytes(), "loss differs from mode %s" % first[0]
        assert lse is None or first[2] is None or np.array_equal(lse.view(np.int32), first[2].view(np.int32)), \
            "lse differs from mode %s" % first[0]
        for k in R.ARRAYS:
            assert np.array_equal(after[k], first[3][k]), "%s differs from mode %s" % (k, first[0])


LONG_CASES = [n for n in R.GEOMETRY_CASES if max([r[1] for r in R.SPECS[n].q_runs + R.SPECS[n].c_runs] or [0]) > R.SEG_CHUNK]


def _modes_of(names):
    return [(n, m) for n in names for m in MODES if not (m in HINTED and n in LONG_CASES)]


# ---- batch sizes and widths: every D at B = 256 and 1024, D = 128 at every B; runs of 1 to 13 -----------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,mode", _modes_of(R.SHAPE_CASES))
def test_shapes(dev, monkeypatch, name, mode, dtype):
    _one_step(dev, monkeypatch, name, dtype, mode)


# ---- the geometry of the sorted occurrence list, at D = 128 and D = 64 --------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,mode", _modes_of(R.GEOMETRY_CASES))
def test_run_geometry(dev, monkeypatch, name, mode, dtype):
    _one_step(dev, monkeypatch, name, dtype, mode)


def test_long_run_cases_are_the_ones_left_out_of_the_hinted_modes():
    for n in R.GEOMETRY_CASES + R.SHAPE_CASES:
        assert R.has_long_run(R.make_case(n)) == (n in LONG_CASES)
    assert len(LONG_CASES) == 10  # run33-64, hot-q, hot-c, hot-both, edges-long at both widths


# ---- a used workspace: the smallest batch right after the largest and the other way round ---------------------------------
@pytest.mark.parametrize("mode", ["sort", "hint0", "side"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("a,b", [("ws-big-D128", "ws-small-D128"), ("ws-small-D128", "ws-big-D128")])
def test_second_step_on_a_used_workspace(dev, monkeypatch, a, b, dtype, mode):
    """B = 2176 then B = 128 (and 128 then 2176) on the same towers: both calls take their workspace from torch's cached
    block, so what the first step left there -- chunk flags, partial rows, the sorted list, gradient rows of another
    geometry -- lies under the second.  The second reference starts from what the device holds after the first step."""
    ref_a = _reference(a, dtype)
    case_b = R.make_second_step(ref_a, b)  # ids that keep the input conditions on the fp64 state after step one
    tables = Tables(ref_a.case, dev)
    loss, lse = tables.step(mode, monkeypatch)
    mid = _check(ref_a, tables, loss, lse, mode)
    case_b = R.with_inputs(case_b, *(Tables.values(mid)[k] for k in R.ARRAYS))
    gap, both = R.input_conditions(case_b)
    assert gap >= R.MIN_NORM_GAP and both and not R.has_long_run(case_b)
    tables.case = case_b
    loss, lse = tables.step(mode, monkeypatch)
    _check(case_b.reference(), tables, loss, lse, mode, before=mid)

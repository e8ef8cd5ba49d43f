"""Plain NumPy reference of ONE in-batch softmax train step of the two towers (in-batch cross entropy + norm-excess
regulariser, gradients, row-sparse Adagrad on both towers) for the one-call step esr_inbatch_train_step_f16x2, the cases
its GPU test runs and the rules the comparison follows.  No GPU, no torch: tests/test_inbatch_step_ref.py checks all of
it on the CPU and tests/test_gpu_inbatch_step_oracle.py runs the kernels against it.

The arithmetic is oracle.stl_head.inbatch_softmax_loss_and_grads + oracle.optim.sparse_adagrad_update (once per tower,
with all occurrences of that tower) and nothing else; this module only strings them together, builds id lists whose SORTED
occurrence list [qid ; Vq + cid] has runs of prescribed lengths at prescribed positions, and holds the tolerance rule:

    kernel error against fp64  <=  4 * e32 + 2^-22,   e32 = error of the SAME oracle run in float32 against fp64

(arrays, lse among them: max |a - b| over the array / max |b|; the loss: relative difference).  The factor 4: the kernels
sum a score, a row of probabilities and a run of gradient rows in other association orders than NumPy does -- all f32
evaluations of the same expression.  The floor covers the f32 storage of a result that the f32 oracle hits by luck.
The step knows nothing of the kernels' chunking; the positions below are named after it (kSegChunk = 32 sorted positions
per chunk of the update, the tower boundary at sorted position B).
"""
import numpy as np

from _triplet_step_ref import _tower, arr_err, bf16_bits, midpoint_distance, run_lengths  # noqa: F401
from oracle import optim as o_optim
from oracle import stl_head as o_stl

LR, EPS, LAM = 0.05, 1e-7, 0.1
BIG_LR = 0.2         # the large-lr family: a row moves by several per cent of its size in one step
BIG_EPS = 1e-3       # the eps family: sqrt(acc + eps) and sqrt(acc) + eps differ by per cents at acc ~ 1e-2
FLOOR = 2.0 ** -22
FACTOR = 4.0
SEG_CHUNK = 32       # kSegChunk
MIN_NORM_GAP = 1e-3  # every | |row| - 1 | of a gathered row
MAX_TIE_FRACTION = 0.01  # bf16 towers: touched elements whose fp64 result is within the bound of a bf16 tie
MAX_TRIES = 20
ARRAYS = ("query", "cand", "query_acc", "cand_acc")
TOWERS = ("query", "cand")
BOUNDED = ARRAYS + ("lse", "loss")


def step_ref(query, cand, query_acc, cand_acc, qid, cid, scale, lam, batch_size, lr, eps, dtype):
    """One whole step in `dtype`.  Returns a dict: loss, lse [B], the four arrays after the step and the boolean masks
    of the rows the step touched (touched_query [Vq], touched_cand [Vc])."""
    qt, ct = np.asarray(query).astype(dtype), np.asarray(cand).astype(dtype)
    qa, ca = np.asarray(query_acc).astype(dtype), np.asarray(cand_acc).astype(dtype)
    qid, cid = np.asarray(qid, np.int64), np.asarray(cid, np.int64)
    loss, lse, gq, gc = o_stl.inbatch_softmax_loss_and_grads(qt[qid], ct[cid], lam, batch_size, scale, dtype)
    qt2, qa2 = o_optim.sparse_adagrad_update(qt, qa, qid, gq, lr, eps, dtype=dtype)
    ct2, ca2 = o_optim.sparse_adagrad_update(ct, ca, cid, gc, lr, eps, dtype=dtype)
    tq, tc = np.zeros(qt.shape[0], bool), np.zeros(ct.shape[0], bool)
    tq[qid] = True
    tc[cid] = True
    return {"loss": loss, "lse": lse, "query": qt2, "cand": ct2, "query_acc": qa2, "cand_acc": ca2,
            "touched_query": tq, "touched_cand": tc}


# ---- id lists whose sorted form has runs where a spec puts them ----------------------------------------------------------
def ids_with_layout(V, n, runs, rng, fill=(1, 2, 3), id_pool=None):
    """int32 [n], shuffled, whose ascending form has, for every (start, length) of `runs`, one id that occupies exactly the
    positions [start, start + length); the positions between are filled with further ids occurring fill[k % len(fill)]
    times each (cut short where an asked run or the end comes first).  Ids ascend with the position; they are a random
    subset of range(V), or the first ones of id_pool."""
    lengths, pos, k = [], 0, 0

    def fill_to(end):
        nonlocal pos, k
        while pos < end:
            c = min(fill[k % len(fill)], end - pos)
            lengths.append(c)
            pos += c
            k += 1
    for start, length in sorted(runs):
        assert start >= pos and length > 0, "runs overlap"
        fill_to(start)
        lengths.append(length)
        pos += length
    assert pos <= n, "runs ask for more than n positions"
    fill_to(n)
    assert len(lengths) <= V, "V too small for this layout (%d runs)" % len(lengths)
    ids = np.sort(rng.choice(V, len(lengths), replace=False)) if id_pool is None else np.asarray(id_pool)[:len(lengths)]
    out = np.repeat(ids, lengths).astype(np.int32)
    rng.shuffle(out)
    return out


def sorted_occurrences(case):
    """(sorted virtual ids, perm) of the occurrence list [qid ; Vq + cid]: a stable argsort on the CPU"""
    v = np.concatenate([case.qid.astype(np.int64), case.Vq + case.cid.astype(np.int64)])
    perm = np.argsort(v, kind="stable")
    return v[perm].astype(np.int32), perm.astype(np.int32)


def sorted_runs(case):
    """[(start position in the sorted list, length, tower 0 / 1, id inside its tower)] of every run, ascending"""
    srt, _ = sorted_occurrences(case)
    starts = np.flatnonzero(np.concatenate([[True], srt[1:] != srt[:-1]]))
    ends = np.concatenate([starts[1:], [srt.size]])
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v = int(srt[s])
        out.append((s, e - s, int(v >= case.Vq), v - case.Vq if v >= case.Vq else v))
    return out


def longest_run(case):
    return max(r[1] for r in sorted_runs(case))


def has_long_run(case):
    """what esr_long_run_hint answers with chunk = kSegChunk: some id occupies more than 32 sorted positions"""
    return longest_run(case) > SEG_CHUNK


def asked_runs(case):
    """the runs the spec asks for, as sorted_runs() reports them: (start, length, tower, id); asserts each is there"""
    runs = {(s, t): (s, n, t, i) for s, n, t, i in sorted_runs(case)}
    out = []
    for tower, asked in ((0, case.spec.q_runs), (1, case.spec.c_runs)):
        for start, length in asked:
            pos = start + tower * case.B  # (the candidate tower's occurrences follow the B of the query tower)
            got = runs.get((pos, tower))
            assert got is not None and got[1] == length, \
                "%s: no run of %d at sorted position %d (tower %d): %r" % (case.spec.name, length, pos, tower, got)
            assert pos % SEG_CHUNK == start % SEG_CHUNK and pos + length <= (tower + 1) * case.B
            out.append(got)
    return out


class Spec:
    """q_runs / c_runs: [(start, length)] in tower-local sorted positions (the candidate tower's are B further on in the
    list).  batch_size defaults to 1.5 B: a step that divides by B is wrong by a half."""

    def __init__(self, name, D, B, q_runs=(), c_runs=(), fill=None, Vq=500, Vc=600, scale=8.0, lam=LAM, lr=LR, eps=EPS,
                 batch_size=None, shared_ids=False):
        self.name, self.D, self.B, self.q_runs, self.c_runs = name, D, B, tuple(q_runs), tuple(c_runs)
        self.fill = fill or ((1, 2, 3) if B <= 384 else (1, 2, 3, 5, 8, 13))
        self.Vq, self.Vc, self.scale, self.lam, self.lr, self.eps = Vq, Vc, float(scale), lam, lr, eps
        self.batch_size = float(1.5 * B if batch_size is None else batch_size)
        self.shared_ids = shared_ids  # run k of either tower carries the id k: the same numbers name rows of both towers


BATCHES = (128, 256, 384, 640, 896, 1024, 2176)   # pass-Q split counts 4, 8, 6, 5, 7, 8, 4; 2 B >= 4096 at the last
WIDTHS = (4, 32, 64, 96, 100, 124, 128)           # below 128: the zero-padded tile, never the merging update
ALL_WIDTH_BATCHES = (256, 1024)
GEOMETRY_WIDTHS = (128, 64)
HOT = ((3, 65), (100, 70), (200, 300))            # runs of 65, 70 and 300, the first one position short of a chunk's end


def shape_specs():
    out = []
    for B in BATCHES:
        for D in (WIDTHS if B in ALL_WIDTH_BATCHES else (128,)):
            out.append(Spec("shape-B%d-D%d" % (B, D), D, B, scale=4 + (B // 128 + D) % 5))  # scales 4 to 8
    return out


def geometry_specs(D):
    B, H = 256, 640
    n = lambda s: "%s-D%d" % (s, D)  # noqa: E731
    return [
        Spec(n("distinct"), D, B, fill=(1,), Vq=300, Vc=400),
        Spec(n("runs2to31"), D, B, fill=(2, 31, 3, 17, 16, 15, 8, 30)),
        Spec(n("run32-a0"), D, B, q_runs=[(64, 32)], c_runs=[(32, 32)]),
        Spec(n("run32-a1"), D, B, q_runs=[(33, 32)], c_runs=[(65, 32)]),
        Spec(n("run32-a31"), D, B, q_runs=[(31, 32)], c_runs=[(95, 32)]),
        Spec(n("run33-64"), D, B, q_runs=[(10, 33), (64, 64)], c_runs=[(7, 64), (100, 33)]),
        Spec(n("hot-q"), D, H, q_runs=HOT),
        Spec(n("hot-c"), D, H, c_runs=HOT),
        Spec(n("hot-both"), D, H, q_runs=HOT, c_runs=HOT),
        # a run that ends at sorted position B - 1, one that starts at B (the tower boundary), one that ends at 2 B - 1
        Spec(n("edges"), D, B, q_runs=[(B - 5, 5)], c_runs=[(0, 7), (B - 9, 9)]),
        Spec(n("edges-long"), D, B, q_runs=[(B - 40, 40)], c_runs=[(0, 40), (B - 70, 70)]),
        # the same numbers in both towers: one id occurs 5 times as a query and 9 times as a candidate -- two rows
        Spec(n("same-id"), D, B, q_runs=[(16, 5)], c_runs=[(16, 9)], shared_ids=True),
        Spec(n("negscale"), D, B, scale=-6.0),
        Spec(n("biglr"), D, B, q_runs=[(40, 12)], c_runs=[(80, 12)], lr=BIG_LR),
        Spec(n("eps"), D, B, eps=BIG_EPS),
    ]


SPECS = {s.name: s for s in shape_specs()}
for _D in GEOMETRY_WIDTHS:
    SPECS.update({s.name: s for s in geometry_specs(_D)})
# two steps in a row on the same towers and the same cached workspace block: the largest batch and the smallest
SPECS["ws-big-D128"] = Spec("ws-big-D128", 128, 2176)
SPECS["ws-small-D128"] = Spec("ws-small-D128", 128, 128)
SHAPE_CASES = [s.name for s in shape_specs()]
GEOMETRY_CASES = [s.name for D in GEOMETRY_WIDTHS for s in geometry_specs(D)]


class Case:
    """the inputs of one step: towers and accumulators (f32 arrays; bf16 cases hold bf16 values), ids, settings"""

    def __init__(self, spec, dtype, seed, query, cand, query_acc, cand_acc, qid, cid):
        self.spec, self.dtype, self.seed = spec, dtype, seed
        self.query, self.cand, self.query_acc, self.cand_acc = query, cand, query_acc, cand_acc
        self.qid, self.cid = qid, cid
        self.scale, self.lam, self.batch_size, self.lr, self.eps = spec.scale, spec.lam, spec.batch_size, spec.lr, spec.eps
        self.D, self.B, self.Vq, self.Vc = spec.D, spec.B, spec.Vq, spec.Vc
        self._reference = None

    def reference(self):
        """the fp64 / f32 oracle of this case and its bounds, computed once"""
        if self._reference is None:
            self._reference = Reference(self)
        return self._reference

    def inputs(self):
        return self.query, self.cand, self.query_acc, self.cand_acc

    def ref(self, dtype, **other):
        """step_ref on this case; `other` replaces settings (lam=0.0, batch_size=...)"""
        s = dict(scale=self.scale, lam=self.lam, batch_size=self.batch_size, lr=self.lr, eps=self.eps)
        s.update(other)
        return step_ref(*self.inputs(), self.qid, self.cid, dtype=dtype, **s)


def input_conditions(case):
    """(smallest | |row| - 1 | of a gathered row, both sides of the kink occur in both towers) -- from the inputs alone"""
    nq = np.linalg.norm(case.query.astype(np.float64)[case.qid], axis=1)
    nc = np.linalg.norm(case.cand.astype(np.float64)[case.cid], axis=1)
    gap = float(min(np.abs(nq - 1.0).min(), np.abs(nc - 1.0).min()))
    both = bool(0 < (nq > 1).sum() < nq.size and 0 < (nc > 1).sum() < nc.size)
    return gap, both


def _ids(spec, rng):
    pool = np.arange(min(spec.Vq, spec.Vc)) if spec.shared_ids else None
    return (ids_with_layout(spec.Vq, spec.B, spec.q_runs, rng, spec.fill, pool),
            ids_with_layout(spec.Vc, spec.B, spec.c_runs, rng, spec.fill, pool))


def _draw(spec, dtype, seed):
    rng = np.random.default_rng([seed, spec.D, spec.B])
    u = rng.standard_normal(spec.D)
    u /= np.linalg.norm(u)
    query, cand = _tower(rng, spec.Vq, spec.D, u), _tower(rng, spec.Vc, spec.D, u)
    if dtype == "bf16":
        query, cand = o_optim.round_bf16(query), o_optim.round_bf16(cand)
    qacc = rng.uniform(0.01, 1.0, query.shape).astype(np.float32)
    cacc = rng.uniform(0.01, 1.0, cand.shape).astype(np.float32)
    return Case(spec, dtype, seed, query, cand, qacc, cacc, *_ids(spec, rng))


def _keeps_conditions(case):
    gap, both = input_conditions(case)
    if not (gap >= MIN_NORM_GAP and both):
        return False
    asked_runs(case)  # (asserts: a layout that is not there is a mistake of this module, not a matter of the seed)
    ref = case.reference()
    if not all(np.all(np.isfinite(ref.r64[k])) for k in BOUNDED):
        return False
    return case.dtype != "bf16" or max(ref.tie_fraction.values()) < MAX_TIE_FRACTION


_made = {}


def make_case(name, dtype="f32", first_seed=0):
    """The case of spec `name` in `dtype` ("f32" / "bf16" towers): the first of the seeds first_seed, first_seed + 1, ...
    that keeps the input conditions -- every gathered row's norm at least 1e-3 away from the regulariser's kink at 1, both
    sides of the kink in both towers, the asked runs where the spec puts them, a finite fp64 reference, and (bf16) under
    1 % of the touched elements near a rounding tie; fails after MAX_TRIES.  Deterministic, made once."""
    key = (name, dtype, first_seed)
    if key not in _made:
        for seed in range(first_seed, first_seed + MAX_TRIES):
            case = _draw(SPECS[name], dtype, seed)
            if _keeps_conditions(case):
                _made[key] = case
                break
        else:
            raise AssertionError("no seed of %d keeps the input conditions of %s/%s" % (MAX_TRIES, name, dtype))
    return _made[key]


def make_second_step(first_ref, name, first_seed=0):
    """The case of a step that FOLLOWS the step of first_ref on the same towers: the ids and settings of spec `name`, the
    towers and accumulators as the fp64 reference leaves them (rounded to the table type) -- the first seed whose ids keep
    the input conditions on those."""
    spec, a = SPECS[name], first_ref.case
    assert (spec.D, spec.Vq, spec.Vc) == (a.D, a.Vq, a.Vc)
    inputs = first_ref.next_inputs()
    for seed in range(first_seed, first_seed + MAX_TRIES):
        case = Case(spec, a.dtype, seed, *inputs, *_ids(spec, np.random.default_rng([seed, spec.D, spec.B, 2])))
        if _keeps_conditions(case):
            return case
    raise AssertionError("no seed of %d keeps the input conditions of %s after %s" % (MAX_TRIES, name, a.spec.name))


def with_inputs(case, query, cand, query_acc, cand_acc):
    """the same step on other towers (what a device holds after an earlier step)"""
    return Case(case.spec, case.dtype, case.seed, query, cand, query_acc, cand_acc, case.qid, case.cid)


# ---- the comparison ----------------------------------------------------------------------------------------------------
def _err(k, a, b):
    return abs(float(a) - float(b)) / abs(float(b)) if k == "loss" else arr_err(a, b)


class Reference:
    """fp64 and f32 oracle of one case and the bounds that follow from them.  For bf16 towers `expect_bits` are the bf16
    bit patterns of round_bf16(fp64 result) and `near_tie` marks the elements whose fp64 value lies within tol_abs of a
    midpoint between two neighbouring bf16 values."""

    def __init__(self, case):
        self.case = case
        self.r64, r32 = case.ref(np.float64), case.ref(np.float32)
        self.e32 = {k: _err(k, r32[k], self.r64[k]) for k in BOUNDED}
        self.bound = {k: FACTOR * v + FLOOR for k, v in self.e32.items()}
        self.touched = {k: self.r64["touched_" + k] for k in TOWERS}
        if case.dtype == "bf16":
            self.expect_bits, self.near_tie, self.tie_fraction = {}, {}, {}
            for k in TOWERS:
                x = self.r64[k]
                tol_abs = self.bound[k] * float(np.max(np.abs(x)))
                self.expect_bits[k] = bf16_bits(o_optim.round_bf16(x))
                self.near_tie[k] = midpoint_distance(x) <= tol_abs
                self.tie_fraction[k] = float(self.near_tie[k][self.touched[k]].mean())

    def next_inputs(self):
        """what the towers hold after this step (bf16 towers: rounded) -- the inputs of a second step"""
        r = self.r64
        q, c = r["query"], r["cand"]
        if self.case.dtype == "bf16":
            q, c = o_optim.round_bf16(q), o_optim.round_bf16(c)
        return q.astype(np.float32), c.astype(np.float32), r["query_acc"].astype(np.float32), r["cand_acc"].astype(np.float32)


def compare(ref, got, loss, lse=None):
    """The rules of this module applied to what a step left.  got: dict of the four arrays -- f32 arrays, or uint16 bit
    patterns for bf16 towers; lse: f32 [B], or None where a path does not hand it out.  Returns (ratios, failures):
    ratios[k] = error / bound per quantity that has a bound (bf16 towers are compared bit for bit instead), failures =
    list of strings (empty = pass)."""
    case, r64, fails, ratios = ref.case, ref.r64, [], {}
    ratios["loss"] = _err("loss", loss, r64["loss"]) / ref.bound["loss"]
    if lse is not None:
        ratios["lse"] = arr_err(lse, r64["lse"]) / ref.bound["lse"]
    for k in ARRAYS:
        if k in TOWERS and case.dtype == "bf16":
            bits, want = np.asarray(got[k], np.uint16), ref.expect_bits[k]
            diff = bits != want
            # a differing element: its fp64 value within tol_abs of a midpoint, and the neighbour on the other side
            one_ulp = np.abs(bits.astype(np.int32) - want.astype(np.int32)) == 1
            bad = diff & ~(ref.near_tie[k] & one_ulp)
            if bad.any():
                i = tuple(int(v) for v in np.argwhere(bad)[0])
                fails.append("%s: %d elements differ from round_bf16(fp64) away from a tie; first %r got %04x want %04x"
                             % (k, int(bad.sum()), i, int(bits[i]), int(want[i])))
            if ref.tie_fraction[k] >= MAX_TIE_FRACTION:
                fails.append("%s: %.3f of the touched elements are near a bf16 tie (input condition: < 0.01)"
                             % (k, ref.tie_fraction[k]))
        else:
            ratios[k] = arr_err(got[k], r64[k]) / ref.bound[k]
    for k, v in ratios.items():
        if not v <= 1.0:
            fails.append("%s: error / (4 e32 + 2^-22) = %.3f (e32 = %.3g)" % (k, v, ref.e32[k]))
    return ratios, fails

"""Plain NumPy reference of ONE Shop-The-Look train step (triplet hinge + norm-excess regulariser, gradients, row-sparse
Adagrad on both towers) for the one-pass step esr_triplet_train_step, the cases its GPU test runs and the rules the
comparison follows.  No GPU, no torch: tests/test_triplet_step_ref.py checks all of it on the CPU and
tests/test_gpu_triplet_step_oracle.py runs the kernels against it.

The arithmetic is oracle.stl_head.triplet_loss_and_grads + oracle.optim.sparse_adagrad_update and nothing else; this
module only strings them together, builds id lists with a prescribed run structure, and holds the tolerance rule:

    kernel error against fp64  <=  4 * e32 + 2^-22,   e32 = error of the SAME oracle run in float32 against fp64

(arrays: max |a - b| over the array / max |b|, what conftest.rel_err computes; the loss: relative difference).  The
factor 4: the kernel reduces a dot product across lanes and sums a run left to right, NumPy sums pairwise -- both are
f32 evaluations in other association orders.  The floor covers cases where the f32 oracle is exact by luck.  One Adagrad
step moves a row by ~lr = 5e-2 of its size: a gradient row missed or read stale is four orders above the bound.
"""
import numpy as np

from oracle import optim as o_optim
from oracle import stl_head as o_stl

LR, EPS, LAM = 0.05, 1e-7, 0.1
FLOOR = 2.0 ** -22
FACTOR = 4.0
MIN_MARGIN = 1e-3   # every |1 + s.n - s.p| of a case is at least this (an f32 dot product at D <= 1024 errs by ~1e-6)
MIN_NORM_GAP = 1e-3  # every | |row| - 1 | of a gathered row
MAX_TIE_FRACTION = 0.01  # bf16 towers: touched elements whose fp64 result is within the bound of a bf16 tie
MAX_TRIES = 20
ARRAYS = ("scene", "product", "scene_acc", "product_acc")


def step_ref(scene, product, scene_acc, product_acc, sid, pid, nid, lam, batch_size, lr, eps, dtype):
    """One whole step in `dtype`.  Returns a dict: loss, the four arrays after the step, the per-triplet margin
    1 + s.n - s.p and the three row norms (scene, pos, neg) of every triplet."""
    st, pt = np.asarray(scene).astype(dtype), np.asarray(product).astype(dtype)
    sa, pa = np.asarray(scene_acc).astype(dtype), np.asarray(product_acc).astype(dtype)
    sid, pid, nid = (np.asarray(x, np.int64) for x in (sid, pid, nid))
    s, p, n = st[sid], pt[pid], pt[nid]
    loss, gs, gp, gn = o_stl.triplet_loss_and_grads(s, p, n, lam, batch_size, dtype)
    pos_score, neg_score = o_stl.scores(s, p, n, dtype)
    margin = dtype(1.0) + neg_score - pos_score
    norms = tuple(np.sqrt(np.sum(np.square(e), axis=-1, dtype=dtype)) for e in (s, p, n))
    st2, sa2 = o_optim.sparse_adagrad_update(st, sa, sid, gs, lr, eps, dtype=dtype)
    pt2, pa2 = o_optim.sparse_adagrad_update(pt, pa, np.concatenate([pid, nid]), np.concatenate([gp, gn]), lr, eps,
                                             dtype=dtype)
    return {"loss": loss, "scene": st2, "product": pt2, "scene_acc": sa2, "product_acc": pa2, "margin": margin,
            "norms": norms}


# ---- id lists with a prescribed run structure ------------------------------------------------------------------------
def ids_with_runs(V, n, runs, rng, fill=(1,), avoid=()):
    """int32 [n]: id r occurs runs[r] times for every r of the dict `runs`; the other positions are filled with ids that
    are not in `runs` or `avoid`, each occurring fill[k % len(fill)] times (the last one as often as is left); shuffled."""
    out = []
    for r, c in runs.items():
        out += [r] * c
    left = n - len(out)
    assert left >= 0, "runs ask for more than n occurrences"
    taken = set(runs) | set(avoid)
    free = np.array([v for v in rng.permutation(V) if v not in taken], np.int64)
    k = 0
    while left > 0:
        assert k < len(free), "V too small for this run structure"
        c = min(fill[k % len(fill)], left)
        out += [int(free[k])] * c
        left -= c
        k += 1
    out = np.array(out, np.int32)
    rng.shuffle(out)
    return out


def run_lengths(ids):
    """{id: occurrences}"""
    u, c = np.unique(np.asarray(ids), return_counts=True)
    return dict(zip(u.tolist(), c.tolist()))


def _split_pos_neg(rng, B, Vp, pos_runs, neg_runs, fill):
    """pid, nid [B] with the given runs per list; fill ids of the two lists are disjoint (a product row's run is then what
    pos_runs + neg_runs say)."""
    pid = ids_with_runs(Vp, B, pos_runs, rng, fill, avoid=set(neg_runs))
    nid = ids_with_runs(Vp, B, neg_runs, rng, fill, avoid=set(pos_runs) | set(pid.tolist()))
    return pid, nid


def _ids_small_runs(rng, Vs, Vp, B):
    """runs of 1 to 3 in every list"""
    sid = ids_with_runs(Vs, B, {}, rng, fill=(1, 2, 3))
    pid, nid = _split_pos_neg(rng, B, Vp, {}, {}, (1, 2, 3))
    return sid, pid, nid


def _ids_mixed(rng, Vs, Vp, B):
    """Every run class at once (B = 2048): scene rows with 2, 7, 8, 9, 16, 17 and 300 occurrences (id 0 among them: a
    run at sorted position 0), product rows with 2, 7, 8, 9, 16, 17 and 600, two product rows split between the pos and
    the neg list (3 + 4 and 5 + 4), ten triplets with pos == neg, id 5 in both towers; batch order shuffled, so the
    occurrences of a run sit in different workgroups."""
    sid = ids_with_runs(Vs, B, {0: 2, 5: 7, 11: 8, 12: 9, 13: 16, 14: 17, 15: 300}, rng, fill=(1, 1, 2, 3))
    same = list(range(40, 50))  # ten product ids for the pos == neg triplets: each occurs once in both lists
    pos_runs = {5: 2, 21: 7, 22: 8, 23: 9, 24: 16, 25: 17, 26: 350, 30: 3, 31: 5}
    neg_runs = {26: 250, 30: 4, 31: 4}
    pos_runs.update({r: 1 for r in same})
    neg_runs.update({r: 1 for r in same})
    pid, nid = _split_pos_neg(rng, B, Vp, pos_runs, neg_runs, (1, 1, 2, 3))
    # line the ten pos == neg ids up in the same triplets (a swap inside nid keeps every run length)
    for r in same:
        i, j = int(np.flatnonzero(pid == r)[0]), int(np.flatnonzero(nid == r)[0])
        nid[i], nid[j] = nid[j], nid[i]
    return sid, pid, nid


def _ids_last_run(k):
    def make(rng, Vs, Vp, B):
        """product id Vp - 1 occurs k times (the last run of the sorted list ends at n - 1), scene id 0 twice"""
        sid = ids_with_runs(Vs, B, {0: 2}, rng, fill=(1, 2, 3))
        kp = (k + 1) // 2
        pid, nid = _split_pos_neg(rng, B, Vp, {Vp - 1: kp}, {Vp - 1: k - kp} if k > kp else {}, (1, 2, 3))
        return sid, pid, nid
    return make


def _ids_all_runs(k):
    def make(rng, Vs, Vp, B):
        """every run of both towers has exactly k occurrences"""
        assert B % k == 0
        sid = ids_with_runs(Vs, B, {}, rng, fill=(k,))
        prod = ids_with_runs(Vp, 2 * B, {}, rng, fill=(k,))
        return sid, prod[:B].copy(), prod[B:].copy()
    return make


def _ids_uniform(rng, Vs, Vp, B):
    return (rng.integers(0, Vs, B).astype(np.int32), rng.integers(0, Vp, B).astype(np.int32),
            rng.integers(0, Vp, B).astype(np.int32))


# ---- one hot row per tower: the long-run combination of the stamped step -------------------------------------------------
HOT_CHUNK = 8    # kTripChunk: the stamped step cuts a run at the multiples of 8 sorted positions
HOT_GROUPS = 32  # row groups per workgroup of the stamped step (step_geom_few_lanes: 8 lanes per row at D = 128 and D = 6)
# partial sums of the hot run: 2, around the group count, around four times it (the four-in-flight loop's last round),
# and more than 256 continuation chunks (the count of the chunks needs a second pass)
HOT_PARTIALS = (2, HOT_GROUPS - 1, HOT_GROUPS, HOT_GROUPS + 1, 4 * HOT_GROUPS - 1, 4 * HOT_GROUPS, 4 * HOT_GROUPS + 1, 258)
HOT_ALIGN = (0, HOT_CHUNK - 1)


def hot_run_length(partials, align, chunk):
    """The shortest run, its head at `align` inside a chunk, that is cut into `partials` partial sums: the head chunk
    runs to the first chunk boundary at least `chunk` positions on, every further chunk holds `chunk` positions."""
    return chunk + (chunk - align) % chunk + (partials - 2) * chunk + 1


def hot_batch_size(partials, align):
    return hot_run_length(partials, align, HOT_CHUNK) + HOT_CHUNK + 24


def _ids_hot(partials, align):
    def make(rng, Vs, Vp, B):
        """Scene id 1 and product id 1 (in the pos list) occur L times, L cut into `partials` partial sums; `align` scene
        ids 0 sort in front of the scene run, and as many product ids 0 in front of the product run as put ITS head (sorted
        position B + their number) at the other alignment; every other id occurs once."""
        L = hot_run_length(partials, align, HOT_CHUNK)
        other = HOT_ALIGN[1] if align == HOT_ALIGN[0] else HOT_ALIGN[0]
        # (the product run starts elsewhere in its chunk, so its head chunk may hold up to 7 positions more or fewer:
        # its number of partials is `partials` or one off)
        front = (other - B) % HOT_CHUNK
        sid = ids_with_runs(Vs, B, {0: align, 1: L}, rng)
        pid, nid = _split_pos_neg(rng, B, Vp, {0: front, 1: L}, {}, (1,))
        return sid, pid, nid
    return make


def hot_partials(sorted_ids, vid, chunk):
    """(number of partial sums, alignment of the head) of virtual row vid's run in a sorted list"""
    pos = np.flatnonzero(np.asarray(sorted_ids) == vid)
    h, end = int(pos[0]), int(pos[-1]) + 1
    nxt = (h + 2 * chunk - 1) // chunk * chunk
    return 1 + max(0, -(-(end - nxt) // chunk)), h % chunk


class Spec:
    def __init__(self, name, D, B, ids=_ids_small_runs, Vs=300, Vp=400, lam=LAM, batch_size=None, redraw_neg=False):
        self.name, self.D, self.B, self.ids, self.Vs, self.Vp, self.lam = name, D, B, ids, Vs, Vp, lam
        self.batch_size = float(B if batch_size is None else batch_size)
        # uniform ids at a B where SOME margin of a draw is always near the hinge: the neg id of such a triplet is drawn
        # again (a margin depends on its own triplet only) -- still every triplet is compared
        self.redraw_neg = redraw_neg


# section "widths": one D per (VEC, NCH) instantiation and lane count
WIDTHS_VEC4 = (4, 12, 100, 128, 256, 260, 512, 520, 1024)
WIDTHS_SCALAR = (1, 6, 63, 70, 130, 255)
WIDTHS = WIDTHS_VEC4 + WIDTHS_SCALAR
WIDTHS_VEC8 = tuple(D for D in WIDTHS if D % 8 == 0) + (12,)  # 12: ESR_BF16_VEC8 falls back to 4-element chunks
RUN_WIDTHS = (128, 6)


def _run_specs(D):
    big = dict(Vs=1500, Vp=3000)
    return [
        Spec("mixed-D%d" % D, D, 2048, _ids_mixed, **big),
        Spec("last2-D%d" % D, D, 384, _ids_last_run(2)),
        Spec("last8-D%d" % D, D, 384, _ids_last_run(8)),
        Spec("last9-D%d" % D, D, 384, _ids_last_run(9)),
        Spec("all9-D%d" % D, D, 1152, _ids_all_runs(9)),   # 128 + 256 runs of 9: 384 long runs, long_heads full
        Spec("all8-D%d" % D, D, 1152, _ids_all_runs(8)),   # no long run at all
        Spec("B1-D%d" % D, D, 1),
        Spec("B2-D%d" % D, D, 2),
        Spec("B33-D%d" % D, D, 33),
        Spec("reg0-D%d" % D, D, 384, lam=0.0),
        Spec("bs100-D%d" % D, D, 384, batch_size=100.0),
    ]


SPECS = {}
for _D in WIDTHS:
    SPECS["width-D%d" % _D] = Spec("width-D%d" % _D, _D, 384)
for _D in RUN_WIDTHS:
    for _s in _run_specs(_D):
        SPECS[_s.name] = _s
for _D in (253, 254):  # just inside the argument check's limit for scalar rows (255 and 1024 are widths above)
    SPECS["edge-D%d" % _D] = Spec("edge-D%d" % _D, _D, 64)
SPECS["gridstride-D128"] = Spec("gridstride-D128", 128, 32768, _ids_uniform, Vs=40000, Vp=40000, redraw_neg=True)
# two batches in a row on the same towers and plan buffer: long runs first, none in the second
SPECS["twostep-a-D128"] = Spec("twostep-a-D128", 128, 1152, _ids_all_runs(9))
SPECS["twostep-b-D128"] = Spec("twostep-b-D128", 128, 1152, _ids_all_runs(8))  # (ids only: make_second_step)

RUN_CASES = [s.name[:-5] for s in _run_specs(128)]  # names without the "-D128"
HOT_CASES = ["hot-P%d-a%d" % (p, a) for p in HOT_PARTIALS for a in HOT_ALIGN]
for _D in RUN_WIDTHS:
    for _p in HOT_PARTIALS:
        for _a in HOT_ALIGN:
            _B = hot_batch_size(_p, _a)
            _n = "hot-P%d-a%d-D%d" % (_p, _a, _D)
            SPECS[_n] = Spec(_n, _D, _B, _ids_hot(_p, _a), Vs=_B + 64, Vp=2 * _B + 64)


# ---- towers ------------------------------------------------------------------------------------------------------------
def _tower(rng, V, D, u):
    """[V, D] f32 rows: norms in [0.5, 0.96] or [1.04, 1.6] (half each: regulariser live / dead, and well away from 1
    even after a rounding to bf16), directions +-0.9 u + noise -- scores of either sign and size ~1, so the hinge is
    live for some triplets and dead for others."""
    z = rng.standard_normal((V, D))
    z /= np.maximum(np.linalg.norm(z, axis=1, keepdims=True), 1e-30)
    sign = rng.choice([-1.0, 1.0], size=(V, 1))
    d = 0.9 * sign * u[None, :] + np.sqrt(1.0 - 0.81) * z
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    big = rng.random(V) < 0.5
    norm = np.where(big, rng.uniform(1.04, 1.6, V), rng.uniform(0.5, 0.96, V))
    return (d * norm[:, None]).astype(np.float32)


class Case:
    """the inputs of one step: towers and accumulators (f32 arrays; bf16 cases hold bf16 values), ids, settings"""

    def __init__(self, spec, dtype, seed, scene, product, scene_acc, product_acc, sid, pid, nid):
        self.spec, self.dtype, self.seed = spec, dtype, seed
        self.scene, self.product, self.scene_acc, self.product_acc = scene, product, scene_acc, product_acc
        self.sid, self.pid, self.nid = sid, pid, nid
        self.lam, self.batch_size, self.lr, self.eps = spec.lam, spec.batch_size, LR, EPS
        self.D, self.B, self.Vs, self.Vp = spec.D, spec.B, spec.Vs, spec.Vp
        self._reference = None

    def reference(self):
        """the fp64 / f32 oracle of this case and its bounds, computed once"""
        if self._reference is None:
            self._reference = Reference(self)
        return self._reference

    def inputs(self):
        return self.scene, self.product, self.scene_acc, self.product_acc

    def ref(self, dtype):
        return step_ref(*self.inputs(), self.sid, self.pid, self.nid, self.lam, self.batch_size, self.lr,
                        self.eps, dtype)

    def touched(self):
        ts, tp = np.zeros(self.Vs, bool), np.zeros(self.Vp, bool)
        ts[self.sid] = True
        tp[self.pid] = True
        tp[self.nid] = True
        return ts, tp


def input_conditions(case):
    """(smallest |margin|, smallest | |row| - 1 |) of the fp64 reference -- from the inputs alone"""
    s = case.scene.astype(np.float64)[case.sid]
    p = case.product.astype(np.float64)[case.pid]
    n = case.product.astype(np.float64)[case.nid]
    margin = 1.0 + (s * n).sum(1) - (s * p).sum(1)
    gaps = [np.abs(np.linalg.norm(e, axis=1) - 1.0).min() for e in (s, p, n)]
    return float(np.abs(margin).min()), float(min(gaps)), margin


def _draw(spec, dtype, seed):
    rng = np.random.default_rng([seed, spec.D, spec.B])
    u = rng.standard_normal(spec.D)
    u /= np.linalg.norm(u)
    scene, product = _tower(rng, spec.Vs, spec.D, u), _tower(rng, spec.Vp, spec.D, u)
    if dtype == "bf16":
        scene, product = o_optim.round_bf16(scene), o_optim.round_bf16(product)
    sacc = rng.uniform(0.05, 0.3, scene.shape).astype(np.float32)
    pacc = rng.uniform(0.05, 0.3, product.shape).astype(np.float32)
    sid, pid, nid = spec.ids(rng, spec.Vs, spec.Vp, spec.B)
    case = Case(spec, dtype, seed, scene, product, sacc, pacc, sid, pid, nid)
    if spec.redraw_neg:
        for _ in range(64):
            bad = np.flatnonzero(np.abs(input_conditions(case)[2]) < MIN_MARGIN)
            if bad.size == 0:
                break
            case.nid[bad] = rng.integers(0, spec.Vp, bad.size).astype(np.int32)
    return case


def make_second_step(first_ref, name, first_seed=0):
    """The case of a step that FOLLOWS the step of first_ref on the same towers: the ids of spec `name`, the towers and
    accumulators as the fp64 reference leaves them (rounded to the table type) -- the first seed whose margins and norms
    keep the input conditions on those."""
    spec, a = SPECS[name], first_ref.case
    assert (spec.D, spec.Vs, spec.Vp) == (a.D, a.Vs, a.Vp)
    inputs = first_ref.next_inputs()
    for seed in range(first_seed, first_seed + MAX_TRIES):
        rng = np.random.default_rng([seed, spec.D, spec.B, 2])
        case = Case(spec, a.dtype, seed, *inputs, *spec.ids(rng, spec.Vs, spec.Vp, spec.B))
        m, g, _ = input_conditions(case)
        if m >= MIN_MARGIN and g >= MIN_NORM_GAP and \
                (a.dtype != "bf16" or max(case.reference().tie_fraction.values()) < MAX_TIE_FRACTION):
            return case
    raise AssertionError("no seed of %d keeps the input conditions of %s after %s" % (MAX_TRIES, name, a.spec.name))


def with_inputs(case, scene, product, scene_acc, product_acc):
    """the same step on other towers (what a device holds after an earlier step)"""
    return Case(case.spec, case.dtype, case.seed, scene, product, scene_acc, product_acc, case.sid, case.pid, case.nid)


_made = {}


def make_case(name, dtype="f32", first_seed=0):
    """The case of spec `name` in `dtype` ("f32" / "bf16" towers): the first of the seeds first_seed, first_seed + 1, ...
    whose fp64 margins and row norms keep the input conditions; fails after MAX_TRIES.  Deterministic."""
    key = (name, dtype, first_seed)
    if key in _made:
        return _made[key]
    spec = SPECS[name]
    seen = []
    for seed in range(first_seed, first_seed + MAX_TRIES):
        case = _draw(spec, dtype, seed)
        m, g, _ = input_conditions(case)
        # (bf16 towers: elements whose fp64 result sits within the bound of a bf16 tie may round either way -- under 1 %)
        ties = max(case.reference().tie_fraction.values()) if dtype == "bf16" and min(m, g) >= MIN_MARGIN else 0.0
        if m >= MIN_MARGIN and g >= MIN_NORM_GAP and ties < MAX_TIE_FRACTION:
            if spec.Vs <= 5000:  # (the large case is used once per dtype: not kept)
                _made[key] = case
            return case
        seen.append((seed, m, g, ties))
    raise AssertionError("no seed of %d keeps the input conditions of %s/%s: %r" % (MAX_TRIES, name, dtype, seen))


# ---- the comparison ----------------------------------------------------------------------------------------------------
def arr_err(a, b):
    """max |a - b| / max |b|  (conftest.rel_err without its log)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-30)) if a.size else 0.0


class Reference:
    """fp64 and f32 oracle of one case and the bounds that follow from them.  For bf16 towers `expect_bits` are the bf16
    bit patterns of round_bf16(fp64 result) and `near_tie` marks the elements whose fp64 value lies within tol_abs of a
    midpoint between two neighbouring bf16 values."""

    def __init__(self, case):
        self.case = case
        self.r64, r32 = case.ref(np.float64), case.ref(np.float32)
        self.e32 = {k: arr_err(r32[k], self.r64[k]) for k in ARRAYS}
        self.e32["loss"] = abs(float(r32["loss"]) - self.r64["loss"]) / abs(self.r64["loss"])
        self.bound = {k: FACTOR * v + FLOOR for k, v in self.e32.items()}
        self.touched = dict(zip(("scene", "product"), case.touched()))
        if case.dtype == "bf16":
            self.expect_bits, self.near_tie, self.tie_fraction = {}, {}, {}
            for k in ("scene", "product"):
                x = self.r64[k]
                tol_abs = self.bound[k] * float(np.max(np.abs(x)))
                self.expect_bits[k] = bf16_bits(o_optim.round_bf16(x))
                self.near_tie[k] = midpoint_distance(x) <= tol_abs
                t = self.touched[k]
                self.tie_fraction[k] = float(self.near_tie[k][t].mean()) if t.any() else 0.0

    def next_inputs(self):
        """what the towers hold after this step (bf16 towers: rounded) -- the inputs of a second step"""
        r = self.r64
        s, p = r["scene"], r["product"]
        if self.case.dtype == "bf16":
            s, p = o_optim.round_bf16(s), o_optim.round_bf16(p)
        return s.astype(np.float32), p.astype(np.float32), r["scene_acc"].astype(np.float32), r["product_acc"].astype(np.float32)


def bf16_bits(x):
    """uint16 bit patterns of values that ARE bf16 numbers"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    assert not np.any(u & 0xFFFF), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def bits_to_f64(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def midpoint_distance(x):
    """distance of every fp64 value to the nearest midpoint between two neighbouring bf16 values"""
    ax = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(ax)
    ulp = np.ldexp(1.0, e - 8)  # spacing of bf16 (8 significant bits) in x's binade
    lo = np.floor(ax / ulp) * ulp
    return np.abs(ax - (lo + 0.5 * ulp))


def compare(ref, got, loss):
    """The rules of this module applied to what a step left.  got: dict of the four arrays -- f32 arrays, or uint16 bit
    patterns for bf16 towers.  Returns (ratios, failures): ratios[k] = error / bound per quantity that has a bound (bf16
    towers are compared bit for bit instead), failures = list of strings (empty = pass)."""
    case, r64, fails, ratios = ref.case, ref.r64, [], {}
    ratios["loss"] = abs(float(loss) - r64["loss"]) / abs(r64["loss"]) / ref.bound["loss"]
    for k in ARRAYS:
        tower = k in ("scene", "product")
        if tower and case.dtype == "bf16":
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

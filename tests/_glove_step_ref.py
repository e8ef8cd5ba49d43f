"""Plain NumPy reference of ONE GloVe train step (loss, gradients, row-sparse Adagrad on the embedding and the bias table)
for the one-pass step esr_glove_train_step, the cases its GPU test runs and the rules the comparison follows.  No GPU, no
torch: tests/test_glove_step_ref.py checks all of it on the CPU and tests/test_gpu_glove_step_oracle.py runs the kernels
against it.

The arithmetic is oracle.glove.loss_and_grads + oracle.glove.row_grads + oracle.optim.sparse_adagrad_update and nothing
else; this module strings them together, builds id lists with a prescribed run structure, a starting state of the
double-buffered table (random stamped location bytes, NaN bits in every dead copy) and holds the tolerance rule, which is
the one of tests/_triplet_step_ref.py (FACTOR, FLOOR and the helpers are imported from there):

    kernel error against fp64  <=  4 * e32 + 2^-22,   e32 = error of the SAME oracle run in float32 against fp64

per quantity (embedding, its accumulator, bias, its accumulator: max |a - b| / max |b| of the table; loss: relative), and
for the four arrays PER TOUCHED ROW as well: the row's largest error over max |b| of the table against 4 * (the f32
oracle's error in that row) + 2^-22 -- a bad row cannot hide behind another row's e32.  The factor 4: the kernel reduces a
dot product across lanes, sums an embedding run left to right in f32 (in reference mode as A - sbar C, A = sum (w r)
partner, C = sum w partner) and a bias run in fp64, NumPy sums pairwise: all are f32 evaluations in other association
orders.  bf16 tables: bit-equal to round_bf16(fp64 result), except where the fp64 value x is within the row's bound t of
a tie: there the neighbour on the other side passes too -- stated as "a bf16 value between round_bf16(x - t) and
round_bf16(x + t)", which is that rule wherever a bf16 ulp is larger than t and is what an f32 evaluation can deliver where
it is not: an element that the step all but cancels (width 260, diagonal: -1.9e-7 in a table of rows of norm ~1, where t
is 1.2e-7 and a bf16 ulp 9e-10) came back two bf16 ulps from round_bf16(fp64), 1.9e-9 or 1 / 60 of its bound.

The loss is a mean over B pairs, so gradients shrink as 1 / B: accumulators are drawn as U(0.05, 0.3) / B^2 and eps is
min(1e-7, 0.015 / B^2), so that at every batch size g^2 is of the accumulator's size (a wrong gradient shows in it) and a
single occurrence moves its row far beyond the bound (input condition below).
"""
import numpy as np

from _triplet_step_ref import (FACTOR, FLOOR, MAX_TIE_FRACTION, MAX_TRIES, arr_err, bf16_bits, bits_to_f64,  # noqa: F401
                               hot_partials, ids_with_runs, midpoint_distance, run_lengths)
from oracle import glove as o_glove
from oracle import optim as o_optim

LR = float(np.float32(0.05))
MODES = ("reference", "diagonal")
KEYS = ("emb", "emb_acc", "bias", "bias_acc")
STAMP = 5                   # the stamp of a single step (1 .. 127)
CHUNK = 32                  # kStepChunk: the step cuts a run at the multiples of 32 sorted positions
RESOLVE_MIN_IDS = 32768     # kResolveMinIds: longer lists take the resolve launch and glove_step_resolved_kernel
FIN_FUSE_MAX_IDS = 8192     # kFinFuseMaxIds: up to here the update kernel's last workgroup can be the finalize step
STAT_BLOCKS = 256           # kStatBlocks / kStatBlocksStep
MIN_CONTRIB = 64.0          # an occurrence's own share of its row's update, in units of the row's bound ...
MIN_CONTRIB_SHARE = 0.99    # ... for at least this share of the occurrences
NAN32, NAN16 = 0x7FC0BEEF, 0x7FC1   # what the dead copy of every row (and every sentinel of the GPU test) holds


def eps_for(B):
    return float(np.float32(min(1e-7, 0.015 / (B * B))))


def step_ref(emb, emb_acc, bias, bias_acc, inputs, target, mode, lr, eps, dtype):
    """One whole step in `dtype`: dict of the loss, the four arrays after the step (bias tables as [V]) and the
    per-occurrence pieces (ids, rows, gb of oracle.glove.row_grads)."""
    e, ea = np.asarray(emb).astype(dtype), np.asarray(emb_acc).astype(dtype)
    b, ba = (np.asarray(x).astype(dtype).reshape(-1, 1) for x in (bias, bias_acc))
    loss, gdot, gs = o_glove.loss_and_grads(e, b, inputs, np.asarray(target).astype(dtype), mode, dtype)
    ids, rows, gb = o_glove.row_grads(e, inputs, gdot, gs, dtype)
    e2, ea2 = o_optim.sparse_adagrad_update(e, ea, ids, rows, lr, eps, dtype=dtype)
    b2, ba2 = o_optim.sparse_adagrad_update(b, ba, ids, gb[:, None], lr, eps, dtype=dtype)
    return {"loss": loss, "emb": e2, "emb_acc": ea2, "bias": b2[:, 0], "bias_acc": ba2[:, 0], "ids": ids, "rows": rows,
            "gb": gb}


# ---- mirror of the row geometry and of the dispatch in launch_glove_step_t ----------------------------------------------
def row_geom(D, vec=None):
    """(vec, nvec, G, nch) of esr_common.h row_geom (vec = None) / row_geom8 (vec = 8)"""
    vec = vec or (4 if D % 4 == 0 else 1)
    nvec, G = D // vec, 1
    while G < nvec and G < 64:
        G *= 2
    return vec, nvec, G, -(-nvec // G)


def dim_supported(D):
    """check_dim: at most four chunks per lane of the 4-element / scalar geometry"""
    return row_geom(D)[3] <= 4


def instantiation(D, dtype="f32", vec8=False, aligned16=True):
    """(VEC, NCH, G) of the update kernel a table of this width reaches (ESR_DISPATCH_ROW_ANY: nch 3 runs as 4)"""
    use8 = vec8 and dtype == "bf16" and D % 8 == 0 and aligned16
    vec, _, G, nch = row_geom(D, 8 if use8 else None)
    assert nch <= 4
    return vec, (1 if nch <= 1 else 2 if nch <= 2 else 4), G


def dispatch(B, D, mode, planned=False, long_runs=-1):
    """The path a step takes (launch_glove_step_t): resolved kernel or in-kernel resolution, finalize fused into the update
    kernel or launched, long-run launch made or not, statistics workgroups, and whether the row groups the list asks for
    outnumber any resident grid (kMaxGrid workgroups: groups then walk slices of several positions)."""
    n = 2 * B
    resolved = n > RESOLVE_MIN_IDS
    if not resolved and not planned:
        long_runs = -1  # the plan is made in line: the step screens for long runs itself
    nstat = min(STAT_BLOCKS, -(-B // 256)) if (resolved or mode == "reference") else 0
    return {"resolved": resolved, "fuse_fin": not resolved and long_runs == 0 and n <= FIN_FUSE_MAX_IDS,
            "long_launch": long_runs != 0, "nstat": nstat, "walk": -(-n // (256 // row_geom(D)[2])) > 2048}


# ---- id lists -----------------------------------------------------------------------------------------------------------
def make_inputs(rng, V, B, runs, fill):
    """int32 [2, B]: id r occurs runs[r] times over both rows (ids_with_runs), and -- what every case contains -- ids 0
    and V - 1, one pair of a token with itself and so a token in both rows: two occurrences of the smallest id that has
    two are lined up in one column (a swap: every run keeps its length)."""
    runs = dict(runs)
    runs.setdefault(0, 2 if V > 1 else 2 * B)
    runs.setdefault(V - 1, 1)
    flat = ids_with_runs(V, 2 * B, runs, rng, fill)
    counts = run_lengths(flat)
    tok = min(r for r, c in counts.items() if c >= 2)
    a, b = (int(p) for p in np.flatnonzero(flat == tok)[:2])
    want = (a + B) % (2 * B)  # the other row of a's column
    flat[b], flat[want] = flat[want], flat[b]
    return flat.reshape(2, B)


def sorted_ids(inputs):
    return np.sort(np.asarray(inputs).reshape(-1), kind="stable")


def hot_runs(L, align):
    """id 1 occurs L times with its head at `align` inside a chunk of the sorted list: 32 - or 31 ids 0 in front"""
    return {0: CHUNK if align == 0 else align, 1: L}


class Spec:
    def __init__(self, name, D, B, V, runs=None, fill=(1, 2, 3)):
        self.name, self.D, self.B, self.V, self.fill = name, D, B, V, fill
        self.runs = dict(runs or {})
        self.eps = eps_for(B)


# one D per (VEC, NCH) instantiation and lane count (the triplet helper's widths) and the widest rows check_dim lets in
WIDTHS_VEC4 = (4, 12, 100, 128, 256, 260, 512, 520, 1024)
WIDTHS_SCALAR = (1, 6, 63, 70, 130, 253, 254, 255)
WIDTHS = WIDTHS_VEC4 + WIDTHS_SCALAR
WIDTHS_VEC8 = tuple(D for D in WIDTHS if D % 8 == 0) + (12,)  # 12: ESR_BF16_VEC8 falls back to 4-element chunks
REFUSED_WIDTHS = (257, 258, 259, 1028)
RUN_WIDTHS = (128, 6)
RUN_V = 1000
HOT_RUNS = [(L, a) for L in (32, 33, 64, 65, 97) for a in (0, CHUNK - 1)]


def _run_specs(D):
    ladder = {10 + k: k for k in range(3, CHUNK + 1)}  # with id 0's pair: every run length 2 .. 32
    out = [Spec("ones-D%d" % D, D, 384, RUN_V, {}, (1,)),       # all runs 1 (but id 0's pair with itself)
           Spec("ladder-D%d" % D, D, 384, RUN_V, ladder, (1,)),
           Spec("lastrun-D%d" % D, D, 384, RUN_V, {RUN_V - 1: 65}, (1, 2, 3))]
    out += [Spec("run%d-a%d-D%d" % (L, a, D), D, 384, RUN_V, hot_runs(L, a), (1, 2, 3)) for L, a in HOT_RUNS]
    return out


SPECS = {}
for _D in WIDTHS:
    SPECS["width-D%d" % _D] = Spec("width-D%d" % _D, _D, 384, 600)
for _D in RUN_WIDTHS:
    for _s in _run_specs(_D):
        SPECS[_s.name] = _s
RUN_CASES = [s.name[:-5] for s in _run_specs(128)]  # names without the "-D128"
# thresholds: 2 B around kFinFuseMaxIds and kResolveMinIds at D = 8, grids beyond the resident count at D = 256, and the
# edges of the statistics workgroups (one per 256 pairs)
for _B in (4096, 4097, 16384, 16385):
    SPECS["thr-B%d" % _B] = Spec("thr-B%d" % _B, 8, _B, 3 * _B)
SPECS["walk-resolved"] = Spec("walk-resolved", 256, 16385, 20000)
SPECS["walk-short"] = Spec("walk-short", 256, 16384, 20000)
SPECS["nstat-B1"] = Spec("nstat-B1", 8, 1, 1)   # one pair of the only token with itself: id 0 = id V - 1
for _B in (255, 257):
    SPECS["nstat-B%d" % _B] = Spec("nstat-B%d" % _B, 8, _B, 600)
THRESHOLD_CASES = ["thr-B4096", "thr-B4097", "thr-B16384", "thr-B16385", "walk-resolved", "walk-short", "nstat-B1",
                   "nstat-B255", "nstat-B257"]
RESOLVED_CASES = [n for n in THRESHOLD_CASES if 2 * SPECS[n].B > RESOLVE_MIN_IDS]


# ---- cases --------------------------------------------------------------------------------------------------------------
class Case:
    """the inputs of one step: the LIVE values of the four arrays (f32; a bf16 case holds bf16 values in emb), the
    location byte of every row, ids, targets and settings"""

    def __init__(self, spec, dtype, mode, seed, emb, emb_acc, bias, bias_acc, loc, inputs, target, stamp=STAMP, lr=LR):
        self.spec, self.dtype, self.mode, self.seed = spec, dtype, mode, seed
        self.emb, self.emb_acc, self.bias, self.bias_acc, self.loc = emb, emb_acc, bias, bias_acc, loc
        self.inputs, self.target, self.stamp, self.lr, self.eps = inputs, target, stamp, lr, spec.eps
        self.D, self.B, self.V = spec.D, spec.B, spec.V
        self._reference = None

    def arrays(self):
        return self.emb, self.emb_acc, self.bias, self.bias_acc

    def ref(self, dtype, mode=None):
        return step_ref(*self.arrays(), self.inputs, self.target, mode or self.mode, self.lr, self.eps, dtype)

    def touched(self):
        t = np.zeros(self.V, bool)
        t[self.inputs.reshape(-1)] = True
        return t

    def reference(self):
        """the fp64 / f32 oracle of this case and its bounds, computed once"""
        if self._reference is None:
            self._reference = Reference(self)
        return self._reference


def draw_loc(rng, V, stamp, below=128):
    """bit 0 random, stamp bits random in 0 .. below - 1 but never `stamp`"""
    s = rng.integers(0, below - 1, V)
    s += s >= stamp
    return ((s << 1) | rng.integers(0, 2, V)).astype(np.uint8)


def draw_batch(spec, rng):
    """(inputs [2, B], target [B]): targets log-uniform in [1, 1000] -- weights min(1, c / 100)^0.75 from 0.03 to 1, pairs
    on both sides of the clip -- and one pair with c exactly 100"""
    inputs = make_inputs(rng, spec.V, spec.B, spec.runs, spec.fill)
    target = np.exp(rng.uniform(0.0, np.log(1000.0), spec.B)).astype(np.float32)
    target[rng.integers(0, spec.B)] = 100.0
    return inputs, target


def _draw(spec, dtype, mode, seed):
    rng = np.random.default_rng([seed, spec.D, spec.B])
    V, D, B = spec.V, spec.D, spec.B
    # rows of norm 0.5 .. 1.5 around +- a common direction: dot products of either sign and of the size of log10(1 + c)
    u = rng.standard_normal(D)
    u /= np.linalg.norm(u)
    z = rng.standard_normal((V, D))
    z /= np.maximum(np.linalg.norm(z, axis=1, keepdims=True), 1e-30)
    d = 0.9 * rng.choice([-1.0, 1.0], size=(V, 1)) * u[None, :] + np.sqrt(0.19) * z
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    emb = (d * rng.uniform(0.5, 1.5, (V, 1))).astype(np.float32)
    if dtype == "bf16":
        emb = o_optim.round_bf16(emb)
    bias = (0.05 * rng.standard_normal(V)).astype(np.float32)
    emb_acc = (rng.uniform(0.05, 0.3, (V, D)) / (B * B)).astype(np.float32)
    bias_acc = (rng.uniform(0.05, 0.3, V) / (B * B)).astype(np.float32)
    loc = draw_loc(rng, V, STAMP)
    inputs, target = draw_batch(spec, rng)
    return Case(spec, dtype, mode, seed, emb, emb_acc, bias, bias_acc, loc, inputs, target)


def input_conditions(case):
    """What make_case asserts, from the fp64 reference alone: dict of
    clip        pairs below, at and above c = 100 exist (B < 3: at) and every target lies in [1, 1000]
    contrib     share of the occurrences whose own term lr * g_occ * rsqrt(acc + eps) of their row's update is, in its
                largest element, at least MIN_CONTRIB times the row's bound: dropping or doubling one is far outside
    ties        bf16 tables: share of the touched elements within the row's bound of a bf16 tie (else 0)"""
    ref, c = case.reference(), case.target
    clip = bool(c.min() >= 1.0 and c.max() <= 1000.0 and (c == 100).any() and
                (case.B < 3 or ((c < 100).any() and (c > 100).any())))
    contrib = float((occurrence_contrib(case) >= MIN_CONTRIB).mean())
    return {"clip": clip, "contrib": contrib, "ties": ref.tie_fraction if case.dtype == "bf16" else 0.0}


def occurrence_contrib(case):
    """[2 B] (occurrence order of oracle.glove.row_grads): the largest element of the occurrence's own term of its row's
    update, in units of the row's bound"""
    ref = case.reference()
    r = ref.r64
    inv = 1.0 / np.sqrt(r["emb_acc"] + case.eps)
    own = np.abs(case.lr * r["rows"] * inv[r["ids"]]).max(axis=1)
    return own / (ref.bound_row["emb"][r["ids"]] * ref.scale["emb"])


def conditions_hold(cond):
    return cond["clip"] and cond["contrib"] >= MIN_CONTRIB_SHARE and cond["ties"] < MAX_TIE_FRACTION


_made = {}


def make_case(name, dtype="f32", mode="reference", first_seed=0):
    """The case of spec `name` with `dtype` ("f32" / "bf16") embedding tables in loss mode `mode`: the first of the seeds
    first_seed, first_seed + 1, ... whose fp64 reference keeps the input conditions; fails after MAX_TRIES."""
    key = (name, dtype, mode, first_seed)
    if key in _made:
        return _made[key]
    spec, seen = SPECS[name], []
    for seed in range(first_seed, first_seed + MAX_TRIES):
        case = _draw(spec, dtype, mode, seed)
        cond = input_conditions(case)
        if conditions_hold(cond):
            if spec.V * spec.D <= 1 << 20:  # (the large cases are used once or twice: not kept)
                _made[key] = case
            return case
        seen.append((seed, cond))
    raise AssertionError("no seed of %d keeps the input conditions of %s/%s/%s: %r" % (MAX_TRIES, name, dtype, mode, seen))


def table_values(case, x):
    """fp64 / f32 embedding values as the table holds them (bf16 tables: rounded), f32"""
    return (o_optim.round_bf16(x) if case.dtype == "bf16" else x).astype(np.float32)


def next_case(prev, name, arrays=None, loc=None, first_seed=0):
    """The case of a step that FOLLOWS the step of `prev` (a Case) on the same tables: ids and targets of spec `name`, the
    next stamp, and as values `arrays` / `loc` (what a device holds) or what prev's fp64 reference leaves -- the first
    seed whose conditions hold on those."""
    spec = SPECS[name]
    assert (spec.D, spec.V, spec.B) == (prev.D, prev.V, prev.B)
    if arrays is None:
        r = prev.reference().r64
        arrays = (table_values(prev, r["emb"]),) + tuple(r[k].astype(np.float32) for k in KEYS[1:])
        loc = loc_after(prev.loc, prev.touched(), prev.stamp)
    for seed in range(first_seed, first_seed + MAX_TRIES):
        rng = np.random.default_rng([seed, spec.D, spec.B, 2])
        case = Case(spec, prev.dtype, prev.mode, seed, *arrays, loc, *draw_batch(spec, rng), stamp=prev.stamp + 1)
        if conditions_hold(input_conditions(case)):
            return case
    raise AssertionError("no seed of %d keeps the input conditions of %s after %s" % (MAX_TRIES, name, prev.spec.name))


def with_state(case, arrays, loc, stamp=None):
    """the same batch on other table contents (what a device holds after an earlier step)"""
    return Case(case.spec, case.dtype, case.mode, case.seed, *arrays, loc, case.inputs, case.target,
                stamp=case.stamp if stamp is None else stamp, lr=case.lr)


def loc_after(loc, touched, stamp):
    """the bytes a step leaves: a touched row's bit 0 flipped and its stamp this step's; every other byte as it was"""
    out = loc.copy()
    out[touched] = (stamp << 1) | ((loc[touched] & 1) ^ 1)
    return out


# ---- the state of the double-buffered table, as bit patterns ------------------------------------------------------------
def to_bits(x, bf16=False):
    return bf16_bits(x) if bf16 else np.ascontiguousarray(x, np.float32).view(np.uint32)


def from_bits(bits):
    bits = np.asarray(bits)
    if bits.dtype == np.uint16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


class State:
    """What a device holds, as bit patterns: emb[0] / emb[1] the two buffers ([V, D] uint32, or uint16 for bf16 tables),
    loc [V] uint8, emb_acc [V, D], bias and bias_acc [V] uint32."""

    def __init__(self, emb0, emb1, loc, emb_acc, bias, bias_acc):
        self.emb, self.loc, self.emb_acc, self.bias, self.bias_acc = [emb0, emb1], loc, emb_acc, bias, bias_acc

    def copy(self):
        return State(self.emb[0].copy(), self.emb[1].copy(), self.loc.copy(), self.emb_acc.copy(), self.bias.copy(),
                     self.bias_acc.copy())

    def live(self):
        """(emb, emb_acc, bias, bias_acc) values, every row read from the buffer bit 0 of its byte names"""
        raw = np.where((self.loc & 1).astype(bool)[:, None], self.emb[1], self.emb[0])
        return from_bits(raw), from_bits(self.emb_acc), from_bits(self.bias), from_bits(self.bias_acc)


def initial_state(case):
    """the live value in the buffer bit 0 names, NaN bits in the dead copy of EVERY row"""
    bf16 = case.dtype == "bf16"
    live = to_bits(case.emb, bf16)
    dead = np.full_like(live, NAN16 if bf16 else NAN32)
    one = (case.loc & 1).astype(bool)[:, None]
    return State(np.where(one, dead, live), np.where(one, live, dead), case.loc.copy(), to_bits(case.emb_acc),
                 to_bits(case.bias), to_bits(case.bias_acc))


def state_after(case, before, r):
    """the state a step that computed `r` (a step_ref dict) leaves on `before`"""
    bf16, t = case.dtype == "bf16", case.touched()
    new = to_bits(table_values(case, r["emb"]), bf16)
    out = before.copy()
    to1 = t & ((before.loc & 1) == 0)  # lived in buffer 0: the new value goes to buffer 1
    to0 = t & ((before.loc & 1) == 1)
    out.emb[1][to1], out.emb[0][to0] = new[to1], new[to0]
    out.loc = loc_after(before.loc, t, case.stamp)
    out.emb_acc, out.bias, out.bias_acc = (to_bits(r[k].astype(np.float32)) for k in KEYS[1:])
    return out


# ---- the comparison -----------------------------------------------------------------------------------------------------
def _rows(x):
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape[0], -1)


def row_err(a, b):
    """per row: max |a - b| of the row / max |b| of the table"""
    return np.max(np.abs(_rows(a) - _rows(b)), axis=1) / max(float(np.max(np.abs(b))), 1e-30)


class Reference:
    """fp64 and f32 oracle of one case (or of a chain of steps: r64 / r32 / touched given) and the bounds that follow:
    bound[k] for the table and the loss, bound_row[k][row] per row.  bf16 tables: expect_bits = round_bf16(fp64 result),
    near_tie = the elements whose fp64 value lies within the row's bound of a midpoint between two bf16 neighbours,
    bf16_lo / bf16_hi = round_bf16(fp64 result -+ the row's bound): what a value within the bound can round to."""

    def __init__(self, case, r64=None, r32=None, touched=None):
        self.case = case
        self.r64 = r64 = r64 or case.ref(np.float64)
        r32 = r32 or case.ref(np.float32)
        self.touched = case.touched() if touched is None else touched
        self.e32 = {k: arr_err(r32[k], r64[k]) for k in KEYS}
        self.e32["loss"] = abs(float(r32["loss"]) - float(r64["loss"])) / abs(float(r64["loss"]))
        self.bound = {k: FACTOR * v + FLOOR for k, v in self.e32.items()}
        self.scale = {k: float(np.max(np.abs(r64[k]))) for k in KEYS}
        self.bound_row = {k: FACTOR * row_err(r32[k], r64[k]) + FLOOR for k in KEYS}
        if case.dtype == "bf16":
            x = r64["emb"]
            self.expect_bits = bf16_bits(o_optim.round_bf16(x))
            tol = (self.bound_row["emb"] * self.scale["emb"])[:, None]
            self.near_tie = midpoint_distance(x) <= tol
            self.bf16_lo, self.bf16_hi = o_optim.round_bf16(x - tol), o_optim.round_bf16(x + tol)
            self.tie_fraction = float(self.near_tie[self.touched].mean())


def compare_values(ref, got, loss, fails=None):
    """The tolerance rule applied to the values a step left.  got: dict of the four arrays -- f32 values; "emb" as uint16
    bit patterns for bf16 tables.  Returns (ratios, failures): ratios[k] = error / bound of the table, ratios[k + "/row"]
    = the largest error / bound of a touched row (a bf16 embedding is compared bit for bit instead), failures = list of
    strings (empty = pass)."""
    case, r64, ratios = ref.case, ref.r64, {}
    fails = [] if fails is None else fails
    ratios["loss"] = abs(float(loss) - float(r64["loss"])) / abs(float(r64["loss"])) / ref.bound["loss"]
    t = ref.touched
    for k in KEYS:
        if k == "emb" and case.dtype == "bf16":
            bits, want = np.asarray(got[k], np.uint16), ref.expect_bits
            v = bits_to_f64(bits)
            bad = (bits != want) & ~((v >= ref.bf16_lo) & (v <= ref.bf16_hi))
            if bad.any():
                i = tuple(int(v) for v in np.argwhere(bad)[0])
                fails.append("emb: %d elements differ from round_bf16(fp64) away from a tie; first %r got %04x want %04x"
                             % (int(bad.sum()), i, int(bits[i]), int(want[i])))
            if ref.tie_fraction >= MAX_TIE_FRACTION:
                fails.append("emb: %.3f of the touched elements are near a bf16 tie (input condition: < 0.01)"
                             % ref.tie_fraction)
            continue
        ratios[k] = arr_err(got[k], r64[k]) / ref.bound[k]
        per_row = row_err(got[k], r64[k]) / ref.bound_row[k]
        ratios[k + "/row"] = float(np.max(per_row[t])) if t.any() else 0.0
    for k, v in ratios.items():
        if not v <= 1.0:
            fails.append("%s: error / (4 e32 + 2^-22) = %.3f (table e32 = %.3g)" % (k, v, ref.e32[k.split("/")[0]]))
    return ratios, fails


def compare(ref, before, after, loss):
    """Everything a step must have left, from the State before and after it: the bytes (a touched row's bit 0 flipped and
    its stamp the step's, every other byte as it was), bit for bit both copies of an untouched row, the copy a touched
    row was read from and the untouched rows of the other arrays, and -- read from the buffer a touched row had to move
    to -- the values within the tolerance rule.  Returns (ratios, failures)."""
    case, t, fails = ref.case, ref.touched, []
    bit = (before.loc & 1).astype(bool)
    want = loc_after(before.loc, t, case.stamp)
    bad = np.flatnonzero(after.loc != want)
    if bad.size:
        r = int(bad[0])
        fails.append("loc: %d bytes wrong; first row %d (%s) was %02x is %02x want %02x"
                     % (bad.size, r, "touched" if t[r] else "untouched", int(before.loc[r]), int(after.loc[r]), int(want[r])))
    for buf in (0, 1):
        keep = ~t | (bit == bool(buf))
        if not np.array_equal(after.emb[buf][keep], before.emb[buf][keep]):
            fails.append("emb buffer %d: a copy that the step must not write (untouched row, or the copy a touched row was "
                         "read from) changed" % buf)
    for k in KEYS[1:]:
        if not np.array_equal(getattr(after, k)[~t], getattr(before, k)[~t]):
            fails.append("%s: a row no id names changed" % k)
    moved = np.where(t, ~bit, bit)  # the buffer every row's current value must be in
    raw = np.where(moved[:, None], after.emb[1], after.emb[0])
    got = {"emb": raw if case.dtype == "bf16" else from_bits(raw)}
    got.update({k: from_bits(getattr(after, k)) for k in KEYS[1:]})
    return compare_values(ref, got, loss, fails)


# ---- a chain of steps on the same tables (esr_glove_train_steps) ---------------------------------------------------------
def chain_cases(names, dtype, mode, first_stamp=STAMP):
    """the cases of consecutive steps, each starting from what the fp64 reference of the one before leaves (the starting
    bytes carry stamps below the chain's)"""
    first = make_case(names[0], dtype, mode)
    cases = [with_state(first, first.arrays(), draw_loc(np.random.default_rng(first_stamp), first.V, first_stamp, first_stamp + 1),
                        first_stamp)]
    for name in names[1:]:
        cases.append(next_case(cases[-1], name))
    return cases


def chain_reference(cases):
    """Reference of the LAST state of the chain: fp64 and f32 oracle both chained over all steps (the tables rounded to
    their type between steps); touched = rows any step names.  r64["losses"] = the loss of every step."""
    first, out = cases[0], {}
    for dtype in (np.float64, np.float32):
        arrays, losses = first.arrays(), []
        for c in cases:
            r = step_ref(*arrays, c.inputs, c.target, c.mode, c.lr, c.eps, dtype)
            losses.append(float(r["loss"]))
            arrays = (table_values(c, r["emb"]),) + tuple(r[k].astype(np.float32) for k in KEYS[1:])
        r = dict(r)
        r["losses"] = losses
        out[dtype] = r
    touched = np.zeros(first.V, bool)
    for c in cases:
        touched |= c.touched()
    return Reference(cases[-1], out[np.float64], out[np.float32], touched)


def chain_loc(cases):
    loc = cases[0].loc
    for c in cases:
        loc = loc_after(loc, c.touched(), c.stamp)
    return loc

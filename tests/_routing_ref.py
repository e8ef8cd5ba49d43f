"""CPU-side reference of the unique-row routing plan (esr_unique_by_owner) and of one closed step of the row-sharded
exchange built on it.  No product import: tests/test_routing_ref.py checks all of it on the CPU, tests/test_gpu_routing.py
runs the kernels against it.

    make_keys_case   an occurrence list whose SORTED owner-major keys (key = owner * Lv + local row) have runs of
                     prescribed lengths at prescribed positions, split into 1 to 4 segments with offsets and shuffled
    expected         the five outputs as tests/_cpu_kernels.unique_by_owner states them
    check_plan       the outputs of a plan call against `expected`, and against the contract itself
    Ranks            a world of G ranks inside one process: the two all-to-alls of the exchange are slices and
                     concatenations; everything else is a call on the `kernels` object it is given

The positions are named after the kernels' geometry, which the reference knows nothing of: a thread of the heads /
scatter kernels takes 4 sorted positions, a wave 256, a workgroup (tile) 1024.
"""
import numpy as np
import torch

import _cpu_kernels as cpu
from oracle import optim as o_optim

TILE = 1024        # kUqTile
LIMIT = 1 << 31
OUTPUTS = ("ulocal", "ucounts", "uidx", "sorted_uidx", "perm")


# ---- occurrence lists with a prescribed sorted key layout ---------------------------------------------------------------
def even_bounds(n, world):
    """sorted position at which every owner's keys start (world + 1 entries): the list cut evenly"""
    return [o * n // world for o in range(world + 1)]


def one_owner_bounds(n, world, owner):
    """every position belongs to `owner`: nobody asks anything of the others"""
    return [0] * (owner + 1) + [n] * (world - owner)


def owner_at(bounds, pos):
    return int(np.searchsorted(np.asarray(bounds[1:], np.int64), pos, side="right"))


def _fill(m, fill, k0):
    """run lengths fill[k0], fill[k0 + 1], ... (cyclic) that cover exactly m positions, the last one cut short"""
    if m <= 0:
        return np.zeros(0, np.int64)
    f = np.roll(np.asarray(fill, np.int64), -(k0 % len(fill)))
    lengths = np.tile(f, m // int(f.sum()) + 1)
    c = np.cumsum(lengths)
    k = int(np.searchsorted(c, m, side="left")) + 1
    lengths = lengths[:k].copy()
    lengths[-1] -= c[k - 1] - m
    return lengths


def _distinct(rng, lo, hi, k):
    """k distinct integers of [lo, hi), ascending"""
    m = hi - lo
    assert 0 <= k <= m, "no %d distinct local rows in [%d, %d)" % (k, lo, hi)
    if k == 0:
        return np.zeros(0, np.int64)
    if m <= 4 * k + 16:
        return lo + np.sort(rng.permutation(m)[:k]).astype(np.int64)
    x = np.unique(rng.integers(lo, hi, 2 * k + 16))
    while x.size < k:
        x = np.unique(np.concatenate([x, rng.integers(lo, hi, 2 * k + 16)]))
    return np.sort(rng.choice(x, k, replace=False)).astype(np.int64)


def _locals(rng, Lv, k, edge_locals):
    """k distinct local rows ascending; edge_locals (k >= 4): rows 0, 1, Lv - 2 and Lv - 1 among them"""
    if edge_locals and k >= 4 and Lv >= 4:
        return np.concatenate([[0, 1], _distinct(rng, 2, Lv - 2, k - 4), [Lv - 2, Lv - 1]]).astype(np.int64)
    return _distinct(rng, 0, Lv, k)


def sorted_runs(vid, world, Lv):
    """(start positions, lengths, owners) of the runs of equal keys in the sorted key list of the virtual ids"""
    vid = np.asarray(vid, np.int64)
    sk = np.sort((vid % world) * int(Lv) + vid // world)
    starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]])) if sk.size else np.zeros(0, np.int64)
    lengths = np.diff(np.concatenate([starts, [sk.size]]))
    return starts.astype(np.int64), lengths.astype(np.int64), (sk[starts] // int(Lv)).astype(np.int64)


class KeysCase:
    """segs: int32 arrays (the segments), offsets: their virtual-row offsets, vid: the int64 virtual id of every
    occurrence in list order, runs: the (position, length, owner) asked for, run_pos / run_len / run_owner: every run"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def tensors(self, device="cpu"):
        return [torch.from_numpy(s).to(device) for s in self.segs]


def make_keys_case(n, world, Lv, runs=(), bounds=None, fill=(1, 2, 3), cuts=(), seed=0, edge_locals=False, name=""):
    """runs: [(sorted position, run length, owner)]: one key of that owner occupies exactly those sorted positions.
    bounds: where every owner's keys start in the sorted list (default: an even cut); the positions no run asks for are
    filled, inside every owner's stretch, with further keys occurring fill[k] times each.  Local rows ascend with the
    position and are a random subset of [0, Lv).  cuts: the list positions (after the shuffle) where a new segment
    starts -- 0 to 3 of them, equal cuts give empty segments."""
    n, world, Lv = int(n), int(world), int(Lv)
    assert 1 <= world and Lv >= 1 and world * Lv < LIMIT and 0 <= n < LIMIT
    bounds = list(even_bounds(n, world) if bounds is None else bounds)
    assert len(bounds) == world + 1 and bounds[0] == 0 and bounds[-1] == n and all(np.diff(bounds) >= 0), bounds
    rng = np.random.default_rng([seed, n, world])
    keys, pos_all, len_all, own_all = [], [], [], []
    k = 0
    for o in range(world):
        lo, hi = bounds[o], bounds[o + 1]
        lengths, pos = [], lo
        for start, length, _ in sorted(r for r in runs if r[2] == o):
            assert lo <= pos <= start and length > 0 and start + length <= hi, \
                "%s: run (%d, %d) overlaps another or leaves owner %d's positions [%d, %d)" % (name, start, length, o, lo, hi)
            gap = _fill(start - pos, fill, k)
            k += gap.size
            lengths += [gap, [length]]
            pos = start + length
        gap = _fill(hi - pos, fill, k)
        k += gap.size
        lengths = np.concatenate(lengths + [gap]).astype(np.int64) if hi > lo else np.zeros(0, np.int64)
        assert lengths.sum() == hi - lo
        assert lengths.size <= Lv, "%s: owner %d needs %d distinct rows, Lv = %d" % (name, o, lengths.size, Lv)
        keys.append(np.repeat(o * Lv + _locals(rng, Lv, lengths.size, edge_locals), lengths))
        pos_all.append(lo + np.cumsum(lengths) - lengths)
        len_all.append(lengths)
        own_all.append(np.full(lengths.size, o, np.int64))
    assert all(0 <= r[2] < world for r in runs)
    key = np.concatenate(keys) if n else np.zeros(0, np.int64)
    vid = ((key % Lv) * world + key // Lv)[rng.permutation(n)]
    single = cuts is None      # one segment with offset 0: what the wrapper's single-tensor form takes
    cuts = [] if single else [int(c) for c in cuts]
    assert len(cuts) <= 3 and all(0 <= c <= n for c in cuts) and cuts == sorted(cuts)
    edges = [0] + cuts + [n]
    segs, offsets = [], []
    for s, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        lowest = int(vid[a:b].min()) if b > a else 3 * s
        # a multiple of the world size that leaves no id negative
        offsets.append(0 if single else world * ((lowest // world) // (1 + s % 2)))
        segs.append((vid[a:b] - offsets[-1]).astype(np.int32))
    # what was built, from the segments alone
    built = np.concatenate([s.astype(np.int64) + o for s, o in zip(segs, offsets)])
    assert built.size == n and np.array_equal(built, vid)
    assert n == 0 or (built.min() >= 0 and built.max() < world * Lv)
    assert all(s.size == 0 or s.min() >= 0 for s in segs) and all(o % world == 0 for o in offsets)
    run_pos, run_len, run_owner = (np.concatenate(x) if x else np.zeros(0, np.int64) for x in (pos_all, len_all, own_all))
    got = sorted_runs(built, world, Lv)
    assert all(np.array_equal(a, b) for a, b in zip(got, (run_pos, run_len, run_owner))), "%s: not the layout built" % name
    for start, length, o in runs:
        i = int(np.searchsorted(got[0], start))
        assert i < got[0].size and (got[0][i], got[1][i], got[2][i]) == (start, length, o), \
            "%s: no run of %d of owner %d at sorted position %d" % (name, length, o, start)
    return KeysCase(name=name, n=n, world=world, Lv=Lv, segs=segs, offsets=offsets, vid=built, runs=list(runs),
                    bounds=bounds, run_pos=run_pos, run_len=run_len, run_owner=run_owner, single=single)


# ---- the geometries the plan kernel is run at ----------------------------------------------------------------------------
# list lengths: a thread's four positions; a wave of them; the tiles; where the id sort changes its path (4096 / 4097
# wide keys, 2048 / 2049 and 32768 / 32769 narrow ones, 262144 / 262145 radix with and without segment sums); 257 tiles and
# one position, where a scatter workgroup walks the tile counts a second time
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 32768, 32769, 262144, 262145, 263169)
WORLDS = (1, 2, 3, 5, 7, 8)


def lv_tiny(world):
    return 1                       # ids 0 .. world - 1 only


def lv_mid(world):
    return (1 << 21) // world      # world * Lv <= 2^21: the sort's 32-bit composites


def lv_wide(world):
    return (LIMIT - 1) // world    # the largest key is within 8 of 2^31


def front_bounds(n, world, hi):
    """owner 0 takes the sorted positions [0, hi), the others share the rest evenly"""
    if world == 1:
        return [0, n]
    return [0] + [hi + o * (n - hi) // (world - 1) for o in range(world)]


def seg_cuts(n, variant):
    """one to four segments; an empty one first (2), in the middle (3) and last (4, 5); None: the single-tensor form"""
    return [None, (n // 3,), (0, n // 2), (n // 3, n // 3, 2 * n // 3), (n // 4, n, n), (n // 2, n), ()][variant % 7]


def geometry_specs():
    """[keyword arguments of make_keys_case], one per case, every case named"""
    out = []

    def add(name, n, world, Lv, variant, **kw):
        out.append(dict(name="%s-n%d-w%d" % (name, n, world), n=n, world=world, Lv=Lv(world), cuts=seg_cuts(n, variant),
                        edge_locals=Lv is lv_wide, **kw))
    for i, n in enumerate(SIZES):
        w = WORLDS[i % len(WORLDS)]
        add("mixed-mid", n, w, lv_mid, i)
        w = WORLDS[(i + 3) % len(WORLDS)]
        add("distinct-wide", n, w, lv_wide, i + 2, fill=(1,))
    for i, n in enumerate((262144, 263169)):                         # the long lists with runs, wide keys
        add("mixed-wide", n, (8, 3)[i], lv_wide, i + 1, fill=(1, 2, 3, 5, 8))
    for i, (n, w, lv) in enumerate(((5, 8, lv_tiny), (1025, 8, lv_wide), (4097, 8, lv_tiny), (263169, 8, lv_mid))):
        add("one-id", n, w, lv, i, runs=[(0, n, 5)], bounds=one_owner_bounds(n, w, 5))   # seven owners get nothing
    for i, (n, w) in enumerate(((257, 3), (2049, 5), (32769, 7))):   # every id congruent to one residue
        add("one-residue", n, w, lv_mid, i + 3, bounds=one_owner_bounds(n, w, w - 2))
    for i, (n, w) in enumerate(((5, 5), (1024, 8), (2049, 7), (32769, 3))):  # exactly one distinct row per owner
        b = even_bounds(n, w)
        add("one-per-owner", n, w, lv_tiny, i + 1, runs=[(b[o], b[o + 1] - b[o], o) for o in range(w)], bounds=b)
    run = lambda name, n, w, runs, hi, variant, lv=lv_mid, **kw: add(  # noqa: E731
        name, n, w, lv, variant, runs=[(s, m, 0) for s, m in runs], bounds=front_bounds(n, w, hi), **kw)
    run("run-1023x2", 1025, 2, [(1023, 2)], 1025, 0)                  # across the first tile boundary, no owner behind
    run("run-1023x2", 2049, 3, [(1023, 2), (2047, 2)], 2049, 1, lv=lv_wide)
    run("run-1023x3", 2047, 5, [(1023, 3)], 1500, 2)
    run("run-1020-2052", 4097, 7, [(1020, 1033)], 2500, 3)            # a whole tile inside one run
    run("run-1020-2052", 32768, 8, [(1020, 1033)], 2053, 4, lv=lv_wide)
    run("run-255-257", 1023, 2, [(255, 3)], 600, 5)                   # across a wave of 4-position threads
    run("run4-aligned", 2048, 3, [(8, 4), (252, 4), (1020, 4), (1028, 4)], 1100, 6)
    run("run4-misaligned", 2048, 5, [(13, 4), (254, 4), (1022, 4), (1030, 4), (1035, 4)], 1100, 1)
    for i, (n, w) in enumerate(((1025, 3), (2049, 8), (263169, 2))):  # the last position alone in its tile, a row of its own
        add("last-alone", n, w, lv_mid, i, runs=[(n - 1, 1, w - 1)], fill=(3, 1, 2))
    # rows of their own at the first position of the second and of the third tile; four segments, the second one empty
    add("head-at-tile", 4097, 3, lv_mid, 3, runs=[(1024, 2, 0), (2048, 1, 1)], fill=(1, 2, 3, 2))
    # an owner's first key at a tile's first position (owner 2 gets nothing); in the middle of a thread's four positions
    add("owner-at-tile", 4096, 5, lv_mid, 2, bounds=[0, 1024, 2048, 2048, 3072, 4096], fill=(2, 3))
    add("owner-at-tile", 2049, 2, lv_wide, 3, bounds=[0, 2048, 2049], fill=(1, 2))
    add("owner-in-thread", 4097, 3, lv_mid, 4, bounds=[0, 1026, 2051, 4097], fill=(3, 2))
    add("owner-in-thread", 5, 2, lv_tiny, 5, runs=[(0, 2, 0), (2, 3, 1)], bounds=[0, 2, 5])
    return out


GEOMETRIES = {s["name"]: s for s in geometry_specs()}
_cases = {}


def geometry_case(name):
    """(KeysCase, Plan expected) of a named geometry, made once"""
    if name not in _cases:
        case = make_keys_case(**GEOMETRIES[name])
        _cases[name] = (case, expected_of(case))
    return _cases[name]


# ---- the statement and the contract ----------------------------------------------------------------------------------
class Plan:
    """the five outputs (NumPy) with the list they belong to"""

    def __init__(self, outputs, vid, world, Lv):
        self.ulocal, self.ucounts, self.uidx, self.sorted_uidx, self.perm = outputs
        self.vid, self.world, self.Lv = np.asarray(vid, np.int64), int(world), int(Lv)

    def outputs(self):
        return tuple(getattr(self, k).copy() for k in OUTPUTS)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def expected(segs, offsets, world, Lv):
    """Plan of the list [segs[0] + offsets[0] ; ...] (int32 NumPy arrays): the NumPy statement of the five outputs"""
    out = cpu.unique_by_owner([torch.from_numpy(np.ascontiguousarray(s, np.int32)) for s in segs], world, Lv,
                              offsets=list(offsets))
    vid = np.concatenate([np.asarray(s, np.int64) + int(o) for s, o in zip(segs, offsets)])
    return Plan([_np(t) for t in out], vid, world, Lv)


def expected_of(case):
    return expected(case.segs, case.offsets, case.world, case.Lv)


def check_contract(got, vid, world, Lv):
    """What a plan promises, from the list alone (no statement): raises AssertionError"""
    ulocal, ucounts, uidx, sorted_uidx, perm = (_np(x).astype(np.int64) for x in got)
    vid = np.asarray(vid, np.int64)
    n = vid.size
    assert ucounts.shape == (world,) and (ucounts >= 0).all(), "ucounts %r" % (ucounts,)
    nu = int(ucounts.sum())
    if n == 0:
        assert nu == 0, "an empty list has no rows: ucounts %r" % (ucounts,)
        return
    assert uidx.size == n and sorted_uidx.size == n and perm.size == n and ulocal.size >= nu, "output sizes"
    assert 1 <= nu <= n, "%d distinct rows of %d occurrences" % (nu, n)
    assert np.array_equal(np.sort(perm), np.arange(n)), "perm is not a permutation"
    step = np.diff(sorted_uidx)
    assert sorted_uidx[0] == 0 and ((step == 0) | (step == 1)).all(), "sorted_uidx does not climb from 0 in steps of 0 / 1"
    assert sorted_uidx[-1] == nu - 1, "sorted_uidx ends at %d, ucounts add up to %d" % (sorted_uidx[-1], nu)
    assert np.array_equal(uidx[perm], sorted_uidx), "uidx[perm[p]] != sorted_uidx[p]"
    assert (np.diff(perm)[step == 0] > 0).all(), "perm is not stable: equal keys out of occurrence order"
    ends = np.cumsum(ucounts)
    slice_owner = np.searchsorted(ends, np.arange(nu), side="right")
    ul = ulocal[:nu]
    assert (ul >= 0).all() and (ul < Lv).all(), "local row outside [0, Lv)"
    inside = np.diff(slice_owner) == 0
    assert (np.diff(ul)[inside] > 0).all(), "local rows not strictly ascending inside an owner's slice"
    assert uidx.min() >= 0 and uidx.max() < nu, "uidx outside [0, n_u)"
    back = ul[uidx] * world + slice_owner[uidx]
    bad = np.flatnonzero(back != vid)
    assert bad.size == 0, "occurrence %d reads row %d of owner %d, its id is %d (%d occurrences wrong)" % (
        bad[0], ul[uidx[bad[0]]], slice_owner[uidx[bad[0]]], vid[bad[0]], bad.size)


def check_plan(got, exp):
    """got: the five outputs of a plan call (tensors or arrays, ulocal with or without its tail) for the list of the
    Plan `exp`.  Equal to the statement -- ulocal only as far as sum(ucounts): its tail is unspecified -- and, checked
    on its own, the contract.  Raises AssertionError."""
    ulocal, ucounts, uidx, sorted_uidx, perm = (_np(x) for x in got)
    assert np.array_equal(ucounts, exp.ucounts), "ucounts %r, expected %r" % (ucounts, exp.ucounts)
    nu = int(exp.ucounts.sum())
    assert np.array_equal(ulocal[:nu], exp.ulocal[:nu]), "ulocal differs"
    if exp.vid.size:
        for name, g in (("uidx", uidx), ("sorted_uidx", sorted_uidx), ("perm", perm)):
            e = getattr(exp, name)
            assert g.shape == e.shape, "%s has %r entries, expected %r" % (name, g.shape, e.shape)
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, "%s differs at %d positions, first %d: %d, expected %d" % (name, bad.size, bad[0],
                                                                                          g[bad[0]], e[bad[0]])
    check_contract((ulocal, ucounts, uidx, sorted_uidx, perm), exp.vid, exp.world, exp.Lv)


# ---- a world of G ranks in one process -------------------------------------------------------------------------------
PAD_ROW, PAD_ACC = -77.25, 0.625   # what the shards' padding rows hold


def exact_grads(rng, n, D):
    """gradient rows of multiples of 1/8 in [-4, 4]: sums of up to 2^18 of them are exact in float32 in any order"""
    return (rng.integers(-32, 33, (n, D)) / 8.0).astype(np.float32)


def zipf_ids(rng, n, V, a=1.2):
    return ((rng.zipf(a, n) - 1) % V).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(_np(a), np.float32).view(np.int32)


class Ranks:
    """G ranks that hold the tables `full` (float32 [V_t, D] arrays of one width) row-sharded as ShardedTableGroup lays
    them out: voff[t + 1] = voff[t] + G * ceil(V_t / G), loff = voff / G, rank r's shard of table t = full[t][r::G] --
    padded here to ceil(V_t / G) rows, which no id names.  `kernels` does all the work (esrecsys_amd.ops on a device,
    tests/_cpu_kernels on the CPU); this class only moves data between the ranks."""

    def __init__(self, full, accum, world, kernels, device="cpu"):
        self.G, self.k, self.dev = int(world), kernels, device
        self.V = [int(t.shape[0]) for t in full]
        self.D = int(full[0].shape[1])
        assert all(t.ndim == 2 and t.shape[1] == self.D and a.shape == t.shape for t, a in zip(full, accum))
        G = self.G
        self.voff = [0]
        for v in self.V:
            self.voff.append(self.voff[-1] + G * ((v + G - 1) // G))
        self.loff = [o // G for o in self.voff]
        self.full0 = [np.array(t, np.float32) for t in full]
        self.accum0 = [np.array(a, np.float32) for a in accum]
        self.shards0 = [[self._shard(t, r, PAD_ROW) for t in self.full0] for r in range(G)]
        self.saccum0 = [[self._shard(a, r, PAD_ACC) for a in self.accum0] for r in range(G)]
        self.shards = [[torch.from_numpy(s.copy()).to(device) for s in row] for row in self.shards0]
        self.saccum = [[torch.from_numpy(s.copy()).to(device) for s in row] for row in self.saccum0]

    def _shard(self, t, r, pad):
        out = np.full((-(-t.shape[0] // self.G), t.shape[1]), pad, np.float32)
        mine = t[r::self.G]
        out[:mine.shape[0]] = mine
        return out

    # -- the pieces a test replaces to see the loop fail --
    def return_rows(self, pieces):
        """pieces[o] = the rows owner o sends back to one rank: concatenated owner-major, the order of its ulocal"""
        return torch.cat(pieces)

    def reduce(self, n_u, sorted_uidx, perm, grad_rows):
        """one summed gradient row per distinct row"""
        return self.k.segment_sum_rows(n_u, sorted_uidx, perm, grad_rows.clone())

    def gather(self, o, asked):
        if len(self.V) == 1:
            return self.k.gather_rows(self.shards[o][0], asked)
        return self.k.gather_rows_multi(self.shards[o], self.loff, asked)

    def step(self, ids, grads, lr, eps=1e-7):
        """ids[r] = [(table, int32 array)] the segments of rank r, grads[r] = float32 [n_r, D] one row per occurrence.
        One lookup and one Adagrad update.  Returns per rank a dict: plan (the five outputs), vid, back (the rows that
        came back, in ulocal order), summed (the gradient row per distinct row)."""
        G, k, dev = self.G, self.k, self.dev
        out = []
        for r in range(G):
            segs = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev) for _, a in ids[r]]
            offs = [self.voff[t] for t, _ in ids[r]]
            plan = k.unique_by_owner(segs, G, self.loff[-1], offsets=offs)
            vid = np.concatenate([np.asarray(a, np.int64) + self.voff[t] for t, a in ids[r]])
            out.append({"plan": plan, "vid": vid, "counts": [int(c) for c in _np(plan[1])], "offsets": offs})
        cut = lambda x, counts: list(torch.split(x[:sum(counts)], counts))  # noqa: E731
        asked_from = [cut(o["plan"][0], o["counts"]) for o in out]            # [rank][owner]
        asked = [torch.cat([asked_from[r][o] for r in range(G)]) for o in range(G)]
        served = [cut(self.gather(o, asked[o]), [out[r]["counts"][o] for r in range(G)]) for o in range(G)]
        for r in range(G):
            out[r]["back"] = self.return_rows([served[o][r] for o in range(G)])
            _, _, _, sorted_uidx, perm = out[r]["plan"]
            g = torch.from_numpy(np.ascontiguousarray(grads[r], np.float32)).to(dev)
            out[r]["summed"] = self.reduce(sum(out[r]["counts"]), sorted_uidx, perm, g)
        sent = [cut(out[r]["summed"], out[r]["counts"]) for r in range(G)]
        for o in range(G):
            rows = torch.cat([sent[r][o] for r in range(G)]).contiguous()
            if asked[o].numel() == 0:
                continue
            srt, prm = k.segment_sort(asked[o].contiguous(), self.loff[-1])
            if len(self.V) == 1:
                k.sparse_adagrad(self.shards[o][0], self.saccum[o][0], srt, prm, rows, lr, eps)
            else:
                k.sparse_adagrad_multi(self.shards[o], self.saccum[o], self.loff, srt, prm, rows, lr, eps)
        return out

    def assemble(self, shards):
        """the full tables out of [rank][table] shards (tensors or arrays), padding rows dropped"""
        full = []
        for t, v in enumerate(self.V):
            a = np.empty((v, self.D), np.float32)
            for r in range(self.G):
                a[r::self.G] = _np(shards[r][t])[:len(range(r, v, self.G))]
            full.append(a)
        return full

    def rows_of(self, vid):
        """full0 rows of virtual ids (what a lookup must deliver)"""
        vid = np.asarray(vid, np.int64)
        t = np.searchsorted(np.asarray(self.voff[1:], np.int64), vid, side="right")
        out = np.empty((vid.size, self.D), np.float32)
        for i in range(len(self.V)):
            out[t == i] = self.full0[i][vid[t == i] - self.voff[i]]
        return out


def loop_case(world, count, widths_rows, seed, segment_tables):
    """Inputs of one closed step: tables [(V, D)] of one width, per rank `count` Zipf ids cut into segments over
    segment_tables (table index per segment), gradient rows whose sums are exact.  Returns (full, accum, ids, grads)."""
    rng = np.random.default_rng([seed, world, count])
    full = [(rng.standard_normal((v, d)) * 0.5).astype(np.float32) for v, d in widths_rows]
    accum = [rng.uniform(0.01, 1.0, t.shape).astype(np.float32) for t in full]
    nseg = len(segment_tables)
    sizes = [count // nseg + (1 if s < count % nseg else 0) for s in range(nseg)]
    irng = np.random.default_rng([seed, world, count, 1])   # (the ids do not depend on the tables' width)
    ids = [[(t, zipf_ids(irng, m, widths_rows[t][0])) for t, m in zip(segment_tables, sizes)] for _ in range(world)]
    grads = [exact_grads(rng, count, widths_rows[0][1]) for _ in range(world)]
    return full, accum, ids, grads


def per_table(ids, grads, ntables):
    """all ranks' occurrences table by table: [(ids int64, gradient rows)] -- what an unsharded update is given"""
    out = []
    for t in range(ntables):
        i, g = [], []
        for r, segs in enumerate(ids):
            at = 0
            for tt, a in segs:
                if tt == t:
                    i.append(np.asarray(a, np.int64))
                    g.append(grads[r][at:at + len(a)])
                at += len(a)
        out.append((np.concatenate(i) if i else np.zeros(0, np.int64),
                    np.concatenate(g) if g else np.zeros((0, grads[0].shape[1]), np.float32)))
    return out


def assert_sums_exact(ids, grads, ntables):
    """every per-row sum of the gradient rows, over all ranks, is the same number in float32 as in fp64"""
    for i, g in per_table(ids, grads, ntables):
        if i.size == 0:
            continue
        u, inv = np.unique(i, return_inverse=True)
        s32, s64 = np.zeros((u.size, g.shape[1]), np.float32), np.zeros((u.size, g.shape[1]), np.float64)
        np.add.at(s32, inv, g)
        np.add.at(s64, inv, g.astype(np.float64))
        assert np.array_equal(s32.astype(np.float64), s64) and np.abs(s64).max() < 2.0 ** 20


def oracle_update(full, accum, ids, grads, lr, eps, dtype):
    """ONE Adagrad update of the unsharded tables with all ranks' occurrences: ([tables], [accumulators]) in dtype"""
    tabs, accs = [], []
    for t, (i, g) in enumerate(per_table(ids, grads, len(full))):
        p, a = o_optim.sparse_adagrad_update(full[t], accum[t], i, g, lr, eps, dtype) if i.size else \
            (full[t].astype(dtype), accum[t].astype(dtype))
        tabs.append(p)
        accs.append(a)
    return tabs, accs


def touched_rows(ids, V):
    out = [np.zeros(v, bool) for v in V]
    for segs in ids:
        for t, a in segs:
            out[t][np.asarray(a, np.int64)] = True
    return out

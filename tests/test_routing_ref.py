"""CPU: the reference of the unique-row routing plan (tests/_routing_ref.py) is right before a kernel is measured with it.
The statement on a hand-worked list, every geometry's layout, check_plan against eight wrong plans, and the closed loop
of the in-process ranks on the CPU doubles -- against the unsharded fp64 update, and failing when it is broken."""
import numpy as np
import pytest

import _cpu_kernels as cpu
import _routing_ref as R

# ---- the statement, by hand ----------------------------------------------------------------------------------------------
# world 3, Lv 4: owner = vid % 3, local = vid // 3, key = owner * 4 + local
#   i    0  1  2  3  4  5  6  7  8  9
#   vid  7  2  9  7  0 11  2  4  9  7
#   own  1  2  0  1  0  2  2  1  0  1
#   loc  2  0  3  2  0  3  0  1  3  2
#   key  6  8  3  6  0 11  8  5  3  6
# sorted keys (stable):  0(i4) 3(i2) 3(i8) 5(i7) 6(i0) 6(i3) 6(i9) 8(i1) 8(i6) 11(i5)
# distinct rows:  u0 = (o0, 0)  u1 = (o0, 3)  u2 = (o1, 1)  u3 = (o1, 2)  u4 = (o2, 0)  u5 = (o2, 3)
HAND_VID = np.array([7, 2, 9, 7, 0, 11, 2, 4, 9, 7], np.int32)
HAND = dict(ulocal=[0, 3, 1, 2, 0, 3], ucounts=[2, 2, 2], uidx=[3, 4, 1, 3, 0, 5, 4, 2, 1, 3],
            sorted_uidx=[0, 1, 1, 2, 3, 3, 3, 4, 4, 5], perm=[4, 2, 8, 7, 0, 3, 9, 1, 6, 5])


def test_the_statement_gives_the_hand_worked_plan():
    # one segment; two; four with offsets (multiples of the world size) and an empty one
    for segs, offs in (([HAND_VID], [0]), ([HAND_VID[:4], HAND_VID[4:]], [0, 0]),
                       ([HAND_VID[:3], HAND_VID[3:4] - 6, HAND_VID[4:4], HAND_VID[4:]], [0, 6, 9, 0])):
        exp = R.expected(segs, offs, 3, 4)
        assert np.array_equal(exp.vid, HAND_VID)
        assert exp.ulocal[:6].tolist() == HAND["ulocal"] and exp.ucounts.tolist() == HAND["ucounts"]
        for k in ("uidx", "sorted_uidx", "perm"):
            assert getattr(exp, k).tolist() == HAND[k], k
        R.check_plan(exp.outputs(), exp)
    R.check_contract([np.array(HAND[k]) for k in R.OUTPUTS], HAND_VID, 3, 4)


# ---- the layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_geometry_has_the_layout_it_asks_for(name):
    spec = R.GEOMETRIES[name]
    case, exp = R.geometry_case(name)    # (make_keys_case asserts the runs, the id range and the limits itself)
    n, world, Lv = spec["n"], spec["world"], spec["Lv"]
    assert case.vid.size == n and sum(s.size for s in case.segs) == n and 1 <= len(case.segs) <= 4
    assert all(s.dtype == np.int32 for s in case.segs) and world * Lv < 2 ** 31
    starts, lengths, owners = R.sorted_runs(case.vid, world, Lv)
    for start, length, owner in spec.get("runs", ()):
        i = int(np.searchsorted(starts, start))
        assert (starts[i], lengths[i], owners[i]) == (start, length, owner)
    b = case.bounds
    assert np.array_equal(np.bincount(owners, weights=lengths, minlength=world).astype(np.int64), np.diff(b))
    if spec.get("fill") == (1,):
        assert starts.size == n                                       # all distinct
    assert np.array_equal(exp.ucounts, np.bincount(owners, minlength=world))
    R.check_plan(exp.outputs(), exp)


def test_the_geometries_cover_what_they_claim():
    specs = list(R.GEOMETRIES.values())
    assert {s["n"] for s in specs} >= set(R.SIZES) and {s["world"] for s in specs} == set(R.WORLDS)
    assert len(R.GEOMETRIES) == len(R.geometry_specs())               # no two cases share a name
    nsegs = set()
    for n in R.SIZES:  # every length with narrow and with wide keys: the id sort takes another path for each
        assert {s["Lv"] * s["world"] > (1 << 21) for s in specs if s["n"] == n} == {False, True}, n
    for s in specs:
        c = s["cuts"]
        nsegs.add(1 if c is None else len(c) + 1)
    assert nsegs == {1, 2, 3, 4}
    wide = [R.geometry_case(s["name"])[0] for s in specs if s["Lv"] == R.lv_wide(s["world"]) and s["n"] >= 2048]
    for case in wide:   # local rows 0, 1, Lv - 2, Lv - 1 are asked for and the largest key is world * Lv - 1, the largest
        key = (case.vid % case.world) * case.Lv + case.vid // case.world   # there is: within world + 1 <= 9 of 2^31
        if np.diff(case.bounds)[-1] >= 4 and len(case.runs) == 0:
            assert key.max() == case.world * case.Lv - 1 >= 2 ** 31 - 1 - case.world and key.max() < 2 ** 31
            assert {0, 1, case.Lv - 2, case.Lv - 1} <= set((case.vid // case.world).tolist())
    assert sum(1 for c in wide if not c.runs) >= 4
    empty_first = [s for s in specs if s["cuts"] and s["cuts"][0] == 0]
    empty_last = [s for s in specs if s["cuts"] and s["cuts"][-1] == s["n"]]
    empty_mid = [s for s in specs if s["cuts"] and len(s["cuts"]) == 3 and s["cuts"][0] == s["cuts"][1]]
    assert empty_first and empty_last and empty_mid and any(s["cuts"] is None for s in specs)
    # an owner nobody asks anything of, at world 8 seven of them
    assert any((np.diff(R.geometry_case(s["name"])[0].bounds) == 0).sum() == 7 for s in specs if s["world"] == 8)


# ---- wrong plans -----------------------------------------------------------------------------------------------------------
MUTATED = "head-at-tile-n4097-w3"   # five tiles, three owners, runs of 1 to 3, four segments


def _two_tile_run_case():
    """a run over the sorted positions 1020 .. 2052: position 1024, a tile's first, lies inside it"""
    return R.geometry_case("run-1020-2052-n4097-w7")


def _wrong_plans():
    case, exp = R.geometry_case(MUTATED)
    n, world, Lv = case.n, case.world, case.Lv
    nu = int(exp.ucounts.sum())
    ends = np.cumsum(exp.ucounts)
    out = {}

    def plan(**kw):
        d = dict(zip(R.OUTPUTS, exp.outputs()))
        d.update(kw)
        return tuple(d[k] for k in R.OUTPUTS), exp

    ul = exp.ulocal.copy()                                            # (a) two local rows swapped inside owner 1's slice
    a = int(ends[0]) + 3
    ul[[a, a + 1]] = ul[[a + 1, a]]
    out["a-rows-swapped"] = plan(ulocal=ul)
    case2, exp2 = _two_tile_run_case()
    uc = exp2.ucounts.copy()                                          # (b) the counts of owners 0 and 1 swapped
    assert uc[0] != uc[1]
    uc[[0, 1]] = uc[[1, 0]]
    out["b-counts-swapped"] = ((exp2.ulocal.copy(), uc) + exp2.outputs()[2:], exp2)
    assert exp.sorted_uidx[1024] == exp.sorted_uidx[1023] + 1         # (c) position 1024 starts a run: its head is lost
    su = exp.sorted_uidx.copy()
    su[1024:] -= 1
    ui = np.empty_like(exp.uidx)
    ui[exp.perm] = su                                                 # (uidx follows, so only the missing row shows)
    out["c-tile-head-lost"] = plan(sorted_uidx=su, uidx=ui)
    ui = exp.uidx.copy()                                              # (d) the occurrences of one run one row too far
    u = int(exp.sorted_uidx[2000])
    assert u + 1 < nu
    ui[exp.uidx == u] += 1
    out["d-uidx-off-by-one"] = plan(uidx=ui)
    p = int(np.flatnonzero(np.diff(exp.sorted_uidx) == 0)[7])         # (e) two occurrences of one key swapped in perm
    pm = exp.perm.copy()
    pm[[p, p + 1]] = pm[[p + 1, p]]
    out["e-unstable-perm"] = plan(perm=pm)
    # (f) the plan of somebody who takes owner = vid // Lv, local = vid % Lv: a correct plan of ANOTHER routing
    vid = case.vid
    wrong = R.expected([(vid % Lv * world + vid // Lv).astype(np.int32)], [0], world, Lv)
    assert int(vid.max()) // Lv < world
    out["f-owner-by-division"] = (wrong.outputs(), exp)
    out["g-counts-not-zeroed"] = plan(ucounts=exp.ucounts + np.array([0, 5, 0]))   # (g) added onto what was there
    # (h) the run across the tile boundary at 1024 counted as two rows
    assert exp2.sorted_uidx[1023] == exp2.sorted_uidx[1024] == exp2.sorted_uidx[1020]
    su = exp2.sorted_uidx.copy()
    su[1024:] += 1
    ui = np.empty_like(exp2.uidx)
    ui[exp2.perm] = su
    u = int(exp2.sorted_uidx[1024])
    ul = np.insert(exp2.ulocal, u, exp2.ulocal[u])[:case2.n]
    uc = exp2.ucounts.copy()
    uc[0] += 1                                                        # (the run is owner 0's)
    out["h-run-split-at-tile"] = ((ul, uc, ui, su, exp2.perm.copy()), exp2)
    return out


@pytest.mark.parametrize("which", ["a-rows-swapped", "b-counts-swapped", "c-tile-head-lost", "d-uidx-off-by-one",
                                   "e-unstable-perm", "f-owner-by-division", "g-counts-not-zeroed", "h-run-split-at-tile"])
def test_check_plan_refuses_a_wrong_plan(which):
    got, exp = _wrong_plans()[which]
    R.check_plan(exp.outputs(), exp)                                  # the plan it was made from passes
    with pytest.raises(AssertionError):
        R.check_plan(got, exp)
    with pytest.raises(AssertionError):                               # and the contract alone sees it too
        R.check_contract(got, exp.vid, exp.world, exp.Lv)


def test_check_plan_ignores_the_tail_of_ulocal_and_takes_an_empty_list():
    case, exp = R.geometry_case(MUTATED)
    got = list(exp.outputs())
    got[0][int(exp.ucounts.sum()):] = -12345
    R.check_plan(got, exp)
    empty = R.make_keys_case(0, 3, 7, cuts=(0,), name="empty")
    e = R.expected_of(empty)
    assert e.ucounts.tolist() == [0, 0, 0]
    R.check_plan(e.outputs(), e)
    with pytest.raises(AssertionError):
        R.check_plan((e.ulocal, np.array([0, 1, 0]), e.uidx, e.sorted_uidx, e.perm), e)


# ---- the closed loop on the CPU doubles ------------------------------------------------------------------------------------
LR = 0.05
TABLES = [(4001, 8), (6003, 8)]


class OwnerMinor(R.Ranks):
    """rows come back ordered by local position first and owner second"""

    def return_rows(self, pieces):
        import torch
        order = sorted((i, o) for o, p in enumerate(pieces) for i in range(p.shape[0]))
        return torch.stack([pieces[o][i] for i, o in order]) if order else torch.cat(pieces)


class NoSum(R.Ranks):
    """the first occurrence's gradient row stands for the whole run"""

    def reduce(self, n_u, sorted_uidx, perm, grad_rows):
        import torch
        su, pm = sorted_uidx.numpy(), perm.numpy()
        head = np.concatenate([[True], su[1:] != su[:-1]])
        return grad_rows[torch.from_numpy(pm[head].astype(np.int64))].clone()


def _loop(world, cls=R.Ranks, tables=TABLES, segment_tables=(0, 1, 0), count=1025):
    full, accum, ids, grads = R.loop_case(world, count, tables, 11, segment_tables)
    R.assert_sums_exact(ids, grads, len(tables))
    ranks = cls(full, accum, world, cpu)
    out = ranks.step(ids, grads, LR)
    return ranks, out, (full, accum, ids, grads)


def _lookup_holds(ranks, out):
    return all(np.array_equal(R.bits(o["back"])[R._np(o["plan"][2])], R.bits(ranks.rows_of(o["vid"]))) for o in out)


def _update_holds(ranks, inputs):
    full, accum, ids, grads = inputs
    tabs, accs = R.oracle_update(full, accum, ids, grads, LR, 1e-7, np.float64)
    got_t, got_a = ranks.assemble(ranks.shards), ranks.assemble(ranks.saccum)
    return all(np.array_equal(g, e.astype(np.float32)) for g, e in zip(got_t + got_a, tabs + accs))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_ranks_close_the_loop_on_the_cpu_doubles(world):
    ranks, out, inputs = _loop(world)
    for r, o in enumerate(out):
        exp = R.expected([a for _, a in inputs[2][r]], o["offsets"], world, ranks.loff[-1])
        R.check_plan(o["plan"], exp)
    assert _lookup_holds(ranks, out)
    assert _update_holds(ranks, inputs)
    # rows nobody named, the shards' padding rows among them, keep their bits
    touched = R.touched_rows(inputs[2], ranks.V)
    for r in range(world):
        for t in range(len(ranks.V)):
            keep = np.ones(ranks.shards0[r][t].shape[0], bool)
            mine = touched[t][r::world]
            keep[:mine.size] = ~mine
            assert np.array_equal(R.bits(ranks.shards[r][t])[keep], R.bits(ranks.shards0[r][t])[keep])
            assert np.array_equal(R.bits(ranks.saccum[r][t])[keep], R.bits(ranks.saccum0[r][t])[keep])
            assert keep[mine.size:].all()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_one_table_of_width_one_closes_the_loop_too(world):
    ranks, out, inputs = _loop(world, tables=[(1501, 1)], segment_tables=(0, 0))
    assert _lookup_holds(ranks, out) and _update_holds(ranks, inputs)


@pytest.mark.parametrize("world", [2, 3, 8])
def test_the_loop_fails_when_rows_come_back_owner_minor(world):
    ranks, out, inputs = _loop(world, OwnerMinor)
    assert not _lookup_holds(ranks, out)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_the_loop_fails_when_the_per_row_sum_is_skipped(world):
    ranks, out, inputs = _loop(world, NoSum)
    assert _lookup_holds(ranks, out)
    assert not _update_holds(ranks, inputs)

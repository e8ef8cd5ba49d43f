"""GPU: the unique-row routing plan (esr_unique_by_owner) against its NumPy statement and its contract at every length
where the code changes its way, worlds 1 to 8, and the closed loop of the row-sharded exchange on one device.

The plan.  tests/_routing_ref.py builds occurrence lists whose sorted owner-major keys have runs at prescribed positions
(GEOMETRIES) and check_plan compares the five outputs with the statement and with the contract.  Every output buffer
holds garbage before the call: the blocks of a decoy call, overwritten and released, come back from the caching
allocator; the calls through the C ABI fill their buffers themselves.

    n (world with narrow keys, world * Lv <= 2^21 / world with keys up to 2^31 - 1 - world):
    1 (1/5)  3 (2/7)  4 (3/8)  5 (5/1)  255 (7/2)  256 (8/3)  257 (1/5)  1023 (2/7)  1024 (3/8)  1025 (5/1)  2047 (7/2)
    2048 (8/3)  2049 (1/5)  4096 (2/7)  4097 (3/8)  32768 (5/1)  32769 (7/2)  262144 (8/3)  262145 (1/5)  263169 (2/7)
    and, with runs: 262144 wide at world 8, 263169 wide at world 3; one id n times at world 8 (5, 1025, 4097, 263169);
    one residue at worlds 3, 5, 7; one row per owner at worlds 5, 8, 7, 3; the prescribed runs of the module at worlds
    2, 3, 5, 7, 8.

The closed loop.  _routing_ref.Ranks with esrecsys_amd.ops: worlds 2, 3, 8, 768 / 1025 / 5000 occurrences per rank, two
tables of 4001 and 6003 rows at D = 4, 32, 128, and the GloVe pair [1501, 64] + [1501, 1].  Gradient rows are multiples
of 1/8, so every sum is exact and the update differs from the fp64 oracle only by the f32 evaluation of
p - lr g / sqrt(acc + eps).  Bound: 4 x the largest per-element error of the SAME oracle run in float32, per case, for
the tables and for the accumulators.

    measured on an MI355X, absolute error per element against fp64 (each test prints its own figures):
    tables        f32 oracle 5.8e-08 to 1.14e-07 per case, kernel 5.8e-08 to 1.14e-07; largest kernel error 1.14e-07
                  (w2-n5000-D128, f32 oracle 1.14e-07); kernel / f32 oracle between 0.979 and 1.066 (w2-n768-D4:
                  6.25e-08 against 5.86e-08), equal to three digits in 10 of the 15 cases
    accumulators  f32 oracle 7.7e-06 to 4.48e-03 per case (the hot row's sum squared); the kernel's error is the f32
                  oracle's in every case, ratio 1.000; largest 4.48e-03 (w8-n5000-D32)
    The reassembled tables and accumulators equal the single-device update bit for bit in all 15 cases.
"""
import ctypes

import numpy as np
import pytest
import torch

import _routing_ref as R

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -3
LR, EPS = 0.05, 1e-7
GARBAGE = 0x5A5A5A5A


# ---- the plan against the statement ----------------------------------------------------------------------------------------
def plan_through_ops(dev, case):
    """ops.unique_by_owner on buffers that hold garbage: a decoy call on other ids of the same shapes, its five outputs
    overwritten and released -- the allocator hands the same blocks to the call that counts"""
    from esrecsys_amd import ops
    segs = case.tensors(dev)
    args = (case.world, case.Lv)
    kw = {} if case.single else {"offsets": case.offsets}
    decoy = ops.unique_by_owner(segs[0].flip(0).contiguous() if case.single else [s.flip(0).contiguous() for s in segs],
                                *args, **kw)
    for t in decoy:
        t.fill_(GARBAGE)
    torch.cuda.synchronize()
    del decoy
    return ops.unique_by_owner(segs[0] if case.single else segs, *args, **kw)


@pytest.mark.parametrize("name", list(R.GEOMETRIES))
def test_plan_equals_the_statement(dev, name):
    case, exp = R.geometry_case(name)
    got = plan_through_ops(dev, case)
    assert [t.numel() for t in got] == [case.n, case.world, case.n, case.n, case.n]
    R.check_plan(got, exp)


@pytest.mark.parametrize("name", ["mixed-mid-n5-w5", "distinct-wide-n4097-w8", "mixed-mid-n32769-w7",
                                  "mixed-wide-n263169-w3", "one-id-n263169-w8"])
def test_a_second_call_gives_the_same_bits(dev, name):
    from esrecsys_amd import ops
    case, exp = R.geometry_case(name)
    segs = case.tensors(dev)
    nu = int(exp.ucounts.sum())
    a = [t.clone() for t in ops.unique_by_owner(segs, case.world, case.Lv, offsets=case.offsets)]
    b = ops.unique_by_owner(segs, case.world, case.Lv, offsets=case.offsets)
    for k, x, y in zip(R.OUTPUTS, a, b):
        assert torch.equal(x[:nu], y[:nu]) if k == "ulocal" else torch.equal(x, y), k
    R.check_plan(b, exp)


# ---- the C ABI: arguments, workspace, what is left alone ---------------------------------------------------------------
GUARD = 64   # int32 words behind every output, bytes behind the workspace


class Abi:
    """esr_unique_by_owner called directly on buffers of this test: every output pre-filled, guard words behind each"""

    def __init__(self, dev, case):
        from esrecsys_amd import _lib, ops
        self.lib, self.ops, self.case, self.dev = _lib.load(), ops, case, dev
        n, self.n = case.n, case.n
        self.segs = case.tensors(dev)
        self.need = int(self.lib.esr_unique_by_owner_workspace_bytes(n))
        self.out = [torch.full((max(n, 1) + GUARD,), -7, dtype=torch.int32, device=dev) for _ in range(4)]
        self.ucounts = torch.full((16,), 12345, dtype=torch.int64, device=dev)      # room for a world of 9
        self.ws = torch.full((self.need + GUARD + 16,), 0xA5, dtype=torch.uint8, device=dev)

    def call(self, nseg=None, world=None, Lv=None, counts=None, ptrs=None, ws_bytes=None, ws_shift=0):
        c = self.case
        k = len(self.segs)
        p = [t.data_ptr() for t in self.segs] if ptrs is None else ptrs
        cnt = [t.numel() for t in self.segs] if counts is None else counts
        pad = lambda x: list(x) + [0] * (8 - len(x))  # noqa: E731  (eight slots: a call that reads too far reads zeros)
        ulocal, uidx, sorted_uidx, perm = self.out
        rc = self.lib.esr_unique_by_owner(
            (ctypes.c_void_p * 8)(*pad(p)), (ctypes.c_int64 * 8)(*pad(cnt)), (ctypes.c_int64 * 8)(*pad(c.offsets)),
            k if nseg is None else nseg, c.world if world is None else world, c.Lv if Lv is None else Lv,
            ulocal.data_ptr(), uidx.data_ptr(), sorted_uidx.data_ptr(), perm.data_ptr(), self.ucounts.data_ptr(),
            self.ws.data_ptr() + ws_shift, self.need if ws_bytes is None else ws_bytes, self.ops._stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(bool((t == -7).all()) for t in self.out) and bool((self.ucounts == 12345).all()) and \
            bool((self.ws == 0xA5).all())


def test_bad_arguments_are_refused_and_nothing_is_written(dev):
    case, _ = R.geometry_case("head-at-tile-n4097-w3")
    abi = Abi(dev, case)
    assert len(abi.segs) == 4 and case.world * case.Lv < 2 ** 31

    def refused(code, msg, **kw):
        rc = abi.call(**kw)
        err = abi.lib.esr_last_error()
        assert rc == code and b"esr_unique_by_owner" in err and msg in err, (kw, rc, err)
        assert abi.untouched(), kw

    refused(EINVAL, b"nseg=0", nseg=0)
    refused(EINVAL, b"nseg=5", nseg=5)
    refused(EINVAL, b"world=0", world=0)
    refused(EINVAL, b"world=9", world=9)
    refused(EINVAL, b"bad argument", Lv=0)
    for world in (1, 2, 4, 8):
        refused(EINVAL, b"exceed 2^31", world=world, Lv=(1 << 31) // world)
    refused(EINVAL, b"bad segment 1", counts=[100, -1, 100, 100])
    p = [t.data_ptr() for t in abi.segs]
    assert abi.segs[2].numel() > 0
    refused(EINVAL, b"bad segment 2", ptrs=p[:2] + [None] + p[3:])
    refused(EWORKSPACE, b"workspace", ws_bytes=abi.need - 1)
    refused(EWORKSPACE, b"misaligned", ws_shift=4, ws_bytes=abi.need + 8)
    assert abi.call() == 0 and not abi.untouched()                   # the same buffers, good arguments


@pytest.mark.parametrize("name", ["mixed-mid-n5-w5", "head-at-tile-n4097-w3", "distinct-wide-n4097-w8", "mixed-mid-n32769-w7",
                                  "run-1020-2052-n32768-w8", "mixed-wide-n263169-w3"])
def test_the_stated_workspace_is_enough_and_nothing_behind_it_is_written(dev, name):
    case, exp = R.geometry_case(name)
    abi = Abi(dev, case)
    n = case.n
    assert abi.call() == 0
    assert bool((abi.ws[abi.need:] == 0xA5).all()), "bytes behind the stated workspace were written"
    assert all(bool((t[n:] == -7).all()) for t in abi.out), "words behind an output were written"
    assert bool((abi.ucounts[case.world:] == 12345).all())
    R.check_plan([abi.out[0][:n], abi.ucounts[:case.world]] + [t[:n] for t in abi.out[1:]], exp)   # 12345 is gone


@pytest.mark.parametrize("world", [1, 3, 8])
def test_an_empty_list_zeroes_the_counts_and_touches_nothing_else(dev, world):
    from esrecsys_amd import ops
    case = R.make_keys_case(0, world, 1000, cuts=(0, 0), name="empty")
    abi = Abi(dev, case)
    assert abi.call() == 0
    assert abi.ucounts[:world].tolist() == [0] * world and bool((abi.ucounts[world:] == 12345).all())
    assert all(bool((t == -7).all()) for t in abi.out) and bool((abi.ws == 0xA5).all())
    got = ops.unique_by_owner(case.tensors(dev), world, 1000, offsets=case.offsets)
    assert got[1].tolist() == [0] * world and [t.numel() for t in got] == [0, world, 0, 0, 0]
    R.check_plan(got, R.expected_of(case))


# ---- the closed loop ------------------------------------------------------------------------------------------------------
TWO = lambda D: [(4001, D), (6003, D)]  # noqa: E731
# name -> (world, occurrences per rank, [(rows, width)] of one group, table of every segment)
LOOPS = {
    "w2-n768-D4": (2, 768, TWO(4), (0, 1, 0)), "w2-n1025-D32": (2, 1025, TWO(32), (0, 1, 0)),
    "w2-n5000-D128": (2, 5000, TWO(128), (0, 1, 0)), "w3-n768-D32": (3, 768, TWO(32), (0, 1, 0)),
    "w3-n1025-D128": (3, 1025, TWO(128), (0, 1, 0)), "w3-n5000-D4": (3, 5000, TWO(4), (0, 1, 0)),
    "w8-n768-D128": (8, 768, TWO(128), (0, 1, 0)), "w8-n1025-D4": (8, 1025, TWO(4), (0, 1, 0)),
    "w8-n5000-D32": (8, 5000, TWO(32), (0, 1, 0)),
    # the GloVe pair: the same ids on an embedding table and on a bias table of width 1
    "glove-w2-n1025-D64": (2, 1025, [(1501, 64)], (0, 0)), "glove-w2-n1025-D1": (2, 1025, [(1501, 1)], (0, 0)),
    "glove-w3-n5000-D64": (3, 5000, [(1501, 64)], (0, 0)), "glove-w3-n5000-D1": (3, 5000, [(1501, 1)], (0, 0)),
    "glove-w8-n768-D64": (8, 768, [(1501, 64)], (0, 0)), "glove-w8-n768-D1": (8, 768, [(1501, 1)], (0, 0)),
}
_loops = {}


def loop(dev, name):
    """the step of LOOPS[name] on the device and everything it is compared with, made once"""
    if name in _loops:
        return _loops[name]
    from esrecsys_amd import ops
    world, count, tables, segment_tables = LOOPS[name]
    full, accum, ids, grads = R.loop_case(world, count, tables, 5, segment_tables)   # (seed 5: the pair shares its ids)
    R.assert_sums_exact(ids, grads, len(tables))
    ranks = R.Ranks(full, accum, world, ops, dev)
    out = ranks.step(ids, grads, LR, EPS)
    torch.cuda.synchronize()
    rec = {"ranks": ranks, "out": out, "ids": ids, "grads": grads, "full": full, "accum": accum,
           "tables": ranks.assemble(ranks.shards), "accums": ranks.assemble(ranks.saccum),
           "o64": R.oracle_update(full, accum, ids, grads, LR, EPS, np.float64),
           "o32": R.oracle_update(full, accum, ids, grads, LR, EPS, np.float32)}
    # the library on ONE device: segment_sort + sparse_adagrad of every unsharded table with all ranks' occurrences
    single_t, single_a = [], []
    for t, (i, g) in enumerate(R.per_table(ids, grads, len(tables))):
        tab, acc = torch.from_numpy(full[t].copy()).to(dev), torch.from_numpy(accum[t].copy()).to(dev)
        if i.size:
            srt, prm = ops.segment_sort(torch.from_numpy(i.astype(np.int32)).to(dev), tables[t][0])
            ops.sparse_adagrad(tab, acc, srt, prm, torch.from_numpy(g.copy()).to(dev), LR, EPS)
        single_t.append(tab.cpu().numpy())
        single_a.append(acc.cpu().numpy())
    rec["single"] = (single_t, single_a)
    _loops[name] = rec
    return rec


def test_the_glove_pair_shares_its_ids():
    for a, b in (("glove-w2-n1025-D64", "glove-w2-n1025-D1"), ("glove-w8-n768-D64", "glove-w8-n768-D1")):
        ia, ib = R.loop_case(*LOOPS[a][:3], 5, LOOPS[a][3])[2], R.loop_case(*LOOPS[b][:3], 5, LOOPS[b][3])[2]
        assert all(np.array_equal(x[1], y[1]) for ra, rb in zip(ia, ib) for x, y in zip(ra, rb))


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop_plans_and_lookup(dev, name):
    rec = loop(dev, name)
    ranks = rec["ranks"]
    for r, o in enumerate(rec["out"]):
        R.check_plan(o["plan"], R.expected([a for _, a in rec["ids"][r]], o["offsets"], ranks.G, ranks.loff[-1]))
        back = R.bits(o["back"])
        assert back.shape[0] == sum(o["counts"])
        assert np.array_equal(back[R._np(o["plan"][2])], R.bits(ranks.rows_of(o["vid"]))), "rank %d" % r


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop_sums_per_distinct_row(dev, name):
    rec = loop(dev, name)
    for r, o in enumerate(rec["out"]):
        exp = np.zeros((sum(o["counts"]), rec["ranks"].D), np.float32)
        np.add.at(exp, R._np(o["plan"][2]).astype(np.int64), rec["grads"][r])
        assert np.array_equal(R.bits(o["summed"]), R.bits(exp)), "rank %d" % r


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop_update_against_the_fp64_oracle(dev, name):
    rec = loop(dev, name)
    for what, got, k in (("tables", rec["tables"], 0), ("accumulators", rec["accums"], 1)):
        e32 = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(rec["o32"][k], rec["o64"][k]))
        err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(got, rec["o64"][k]))
        print("%s %s: f32 oracle %.4g  kernel %.4g  ratio %.3f" % (name, what, e32, err, err / e32 if e32 else np.inf))
        assert err <= 4.0 * e32, (what, err, e32)


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop_leaves_other_rows_alone(dev, name):
    rec = loop(dev, name)
    ranks = rec["ranks"]
    touched = R.touched_rows(rec["ids"], ranks.V)
    assert all(0 < t.sum() < t.size for t in touched)
    for r in range(ranks.G):
        for t in range(len(ranks.V)):
            keep = np.ones(ranks.shards0[r][t].shape[0], bool)       # the shard's padding rows stay True
            mine = touched[t][r::ranks.G]
            keep[:mine.size] = ~mine
            assert np.array_equal(R.bits(ranks.shards[r][t])[keep], R.bits(ranks.shards0[r][t])[keep]), (r, t)
            assert np.array_equal(R.bits(ranks.saccum[r][t])[keep], R.bits(ranks.saccum0[r][t])[keep]), (r, t)
    assert any(ranks.shards0[r][t].shape[0] > len(range(r, ranks.V[t], ranks.G))       # (there is a padding row)
               for r in range(ranks.G) for t in range(len(ranks.V)))


@pytest.mark.parametrize("name", list(LOOPS))
def test_loop_equals_the_single_device_update_bit_for_bit(dev, name):
    rec = loop(dev, name)
    for got, exp in zip(rec["tables"] + rec["accums"], rec["single"][0] + rec["single"][1]):
        assert np.array_equal(R.bits(got), R.bits(exp))

"""GPU: lazy Adam (optim.adam(lr, lazy=True)) on the row-sharded and replicated steps.

* esr_adam_catchup_gather, the owner's catch-up-and-serve, equals esr_adam_catchup_rows2 followed by a plain gather byte
  for byte -- served rows, p, mu, nu and last -- for one and two tables, D in {1, 4, 64, 128, 256}, gaps 0, 1, 8, 9 and
  40 across every regime of the long-gap form, duplicate runs and empty input;
* at world 1 through the exchange machinery (ESR_SHARDED_WORLD1_DIRECT=0, ESR_SHARDED_UNIQUE=0), triplet and GloVe steps
  equal a single-device replay with the same public ops bit for bit, tables and optax state, gaps longer than 8 steps
  included;
* at world 2 and 4 over the loopback wire of tests/test_gpu_wire_world.py (the library's own exchange code, uneven
  shards, Zipf ids): flushed and assembled tables, mu and nu match an fp64 dense Adam replay on the unsharded tables;
  sharded_train_steps equals the per-step calls bit for bit; bf16 gradient rows stay inside the bf16 exchange bound;
  the replicated steps keep the replicas bit-identical and match the same replay."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import test_gpu_wire_world as ww  # noqa: E402  (its loopback wire, tables and batches)

pytestmark = pytest.mark.gpu

LR_A = 1e-3  # optax.adam at the reference STL trainer's default learning rate
GAPS = (0, 1, 8, 9, 40)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _equal(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- the kernel ---------------------------------------------------------------------------------------------------------
def _lazy_table(dev, rng, V, D, step):
    p = (rng.standard_normal((V, D)) * 0.1).astype(np.float32)
    mu = (rng.standard_normal((V, D)) * 1e-3).astype(np.float32)
    nu = (10.0 ** rng.uniform(-20, -3, (V, D))).astype(np.float32)  # sqrt(nu) from 1e-10 to 3e-2: both series and the band
    mu[::13] = nu[::13] = 0.0  # rows that never moved
    last = np.array([step - 1 - GAPS[i % len(GAPS)] for i in range(V)], np.int32)
    last[5::17] = step  # rows already current with this step
    return [torch.from_numpy(x).to(dev) for x in (p, mu, nu, last)]


@pytest.mark.parametrize("nt", [1, 2])
@pytest.mark.parametrize("D", [1, 4, 64, 128, 256])
def test_catchup_gather_equals_catchup_rows_then_gather(dev, nt, D):
    from esrecsys_amd import ops
    rng = np.random.default_rng(100 * nt + D)
    step = 50
    Vs = [97, 61][:nt]
    offs = [0] + list(np.cumsum(Vs))
    mine = [_lazy_table(dev, rng, V, D, step) for V in Vs]
    ref = [[x.clone() for x in t] for t in mine]
    vids = rng.integers(0, offs[-1], 700).astype(np.int32)
    vids[:40] = vids[0]               # a long run
    vids[100:700:50] = vids[1]        # a run spread over the whole list (several senders asking for one row)
    vids[200:350] = vids[2]           # a run longer than any row group: its tail served by the copy-only launch
    vt = torch.from_numpy(vids).to(dev)
    srt, perm = ops.segment_sort(vt, int(offs[-1]))
    served = ops.adam_catchup_gather([t[0] for t in mine], [t[1] for t in mine], [t[2] for t in mine],
                                     [t[3] for t in mine], offs, srt, perm, step, LR_A)
    parts = []
    for i, t in enumerate(ref):
        ids = vids[(vids >= offs[i]) & (vids < offs[i + 1])] - offs[i]
        parts.append((t[0], t[1], t[2], t[3], torch.from_numpy(ids.astype(np.int32)).to(dev), 0))
    ops.adam_catchup_rows(parts, step, LR_A)
    if D % 4 == 0:
        expect = ops.gather_rows_multi([t[0] for t in ref], offs, vt)
    else:
        expect = torch.cat([t[0] for t in ref])[vt.long()]
    assert _equal(served, expect)
    for i in range(nt):
        for a, b, what in zip(mine[i], ref[i], ("p", "mu", "nu", "last")):
            assert _equal(a, b), (i, what)
    touched = np.unique(vids)
    assert (torch.cat([t[3] for t in mine]).cpu().numpy()[touched] >= step - 1).all()
    # catch up only: the same state, nothing served
    again = [_lazy_table(dev, np.random.default_rng(100 * nt + D + 1), V, D, step) for V in Vs]
    ref2 = [[x.clone() for x in t] for t in again]
    assert ops.adam_catchup_gather([t[0] for t in again], [t[1] for t in again], [t[2] for t in again],
                                   [t[3] for t in again], offs, srt, None, step, LR_A, serve=False) is None
    ops.adam_catchup_rows([(t[0], t[1], t[2], t[3], p[4], 0) for t, p in zip(ref2, parts)], step, LR_A)
    for a, b in zip(again, ref2):
        assert all(_equal(x, y) for x, y in zip(a, b))


def test_catchup_gather_moves_long_gaps_and_takes_empty_input(dev):
    from esrecsys_amd import ops
    rng = np.random.default_rng(3)
    p, mu, nu, last = _lazy_table(dev, rng, 64, 128, 50)
    p0 = p.clone()
    ids = torch.arange(64, dtype=torch.int32, device=dev)
    srt, perm = ops.segment_sort(ids, 64)
    out = ops.adam_catchup_gather([p], [mu], [nu], [last], [0, 64], srt, perm, 50, LR_A)
    assert _equal(out, p)
    gap40 = [r for r in range(64) if r % len(GAPS) == 4 and r % 13 and (r - 5) % 17]
    assert all(not torch.equal(p[r], p0[r]) for r in gap40)
    assert (last.cpu().numpy() >= 49).all()
    e = torch.empty(0, dtype=torch.int32, device=dev)
    got = ops.adam_catchup_gather([p], [mu], [nu], [last], [0, 64], e, e, 51, LR_A)
    assert tuple(got.shape) == (0, 128)


# ---- world 1 through the exchange machinery ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pg1(dev):
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(free_port())
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    yield dist
    from esrecsys_amd import rccl
    rccl.reset()
    dist.destroy_process_group()


N1 = 12


def _trip_ids(step, rng):
    """Hot rows every step and cold rows at steps 0 and N1 - 1 only: gaps of 11 steps (the long-gap form)."""
    sid = rng.integers(0, 300, ww.B).astype(np.int32)
    pid = rng.integers(0, 500, ww.B).astype(np.int32)
    nid = rng.integers(0, 500, ww.B).astype(np.int32)
    if step in (0, N1 - 1):
        sid[:20] = np.arange(3000, 3020)
        nid[:20] = np.arange(5000, 5020)
    if step % 4 == 1:
        pid[:9] = 7  # duplicates
    return sid, pid, nid


def test_world1_triplet_and_glove_equal_single_device_replay(dev, pg1, monkeypatch):
    from esrecsys_amd import ops, optim, sharded
    monkeypatch.setenv("ESR_SHARDED_WORLD1_DIRECT", "0")
    monkeypatch.setenv("ESR_SHARDED_UNIQUE", "0")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tx = optim.adam(LR_A, lazy=True)
    rng = np.random.default_rng(17)
    batches = [tuple(T(a) for a in _trip_ids(s, rng)) for s in range(N1)]
    st0, pt0 = ww._towers_full()
    V_S, V_P, B = ww.V_S, ww.V_P, ww.B
    gbs = float(B)
    # -- triplet
    towers = sharded.ShardedTableGroup([sharded.RowShardedTable(T(st0), None, V_S), sharded.RowShardedTable(T(pt0), None, V_P)],
                                       kernels=ops)
    assert not towers.unique and not towers.world1_direct
    losses = [sharded.sharded_triplet_step(towers, *b, ww.LAM, gbs, tx) for b in batches]
    assert towers._fused() is None and towers.opt_state["count"] == N1
    tabs = [T(st0), T(pt0)]
    mus, nus = [torch.zeros_like(t) for t in tabs], [torch.zeros_like(t) for t in tabs]
    lasts = [torch.zeros(t.shape[0], dtype=torch.int32, device=dev) for t in tabs]
    offs = [0, V_S, V_S + V_P]
    for t, (sid, pid, nid) in enumerate(batches, 1):
        if t == N1:  # the cold rows: last stepped at step 1, a gap of N1 - 2 > 8 steps
            assert int(lasts[0][3005]) == 1 and int(lasts[1][5005]) == 1
        ops.adam_catchup_rows([(tabs[0], mus[0], nus[0], lasts[0], sid, 0),
                               (tabs[1], mus[1], nus[1], lasts[1], torch.cat([pid, nid]), 0)], t, LR_A)
        vids = ops.concat_offset_ids([sid, pid, nid], [0, V_S, V_S])
        rows = ops.gather_rows_multi(tabs, offs, vids)
        loss, _, _, gs, gp, gn = ops.triplet_fwd_bwd(rows[:B], rows[B:2 * B], rows[2 * B:], None, None, None, B, ww.LAM,
                                                     gbs, with_reg=True, want_grads=True, want_scores=False)
        assert _equal(loss.reshape(-1), losses[t - 1].reshape(-1)), t
        srt, perm = ops.segment_sort(vids, offs[-1])
        ops.sparse_adam_step_lazy(tabs, mus, nus, lasts, offs, srt, perm, torch.cat([gs, gp, gn]), LR_A, t)
    st = towers.opt_state
    for i, g in enumerate(towers.tables):
        for a, b, what in ((g.local, tabs[i], "p"), (st["mu"][i], mus[i], "mu"), (st["nu"][i], nus[i], "nu"),
                           (st["last"][i], lasts[i], "last")):
            assert _equal(a, b), (i, what)
    state = towers.adam_state()
    for i in range(2):
        ops.adam_flush(tabs[i], mus[i], nus[i], lasts[i], N1, LR_A)
        assert _equal(towers.tables[i].local, tabs[i]) and _equal(state["mu"][i], mus[i]) and _equal(state["nu"][i], nus[i])
    assert state["count"] == N1
    # the loop helper at world 1 runs the same machinery (plans of groups of batches, batched owner-side sorts)
    towers2 = sharded.ShardedTableGroup([sharded.RowShardedTable(T(st0), None, V_S),
                                         sharded.RowShardedTable(T(pt0), None, V_P)], kernels=ops)
    losses2 = sharded.sharded_train_steps("triplet", (towers2,), batches, regularization=ww.LAM, global_batch_size=gbs,
                                          lr=tx, plan_group=5)
    towers2.flush()
    assert all(_equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(losses, losses2))
    assert all(_equal(a.local, b.local) for a, b in zip(towers.tables, towers2.tables))
    # -- GloVe (reference-mode loss; bias [V, 1] is its own group)
    e0, b0 = ww._glove_full()
    V, Bg = ww.V_G, ww.B_G
    emb = sharded.ShardedTableGroup([sharded.RowShardedTable(T(e0), None, V)], kernels=ops)
    bia = sharded.ShardedTableGroup([sharded.RowShardedTable(T(b0), None, V)], kernels=ops)
    gb = []
    for s in range(N1):
        inp = rng.integers(0, 200, (2, Bg)).astype(np.int32)
        if s in (0, N1 - 1):
            inp[0, :30] = np.arange(1200, 1230)
        gb.append((T(inp), T(rng.uniform(0.1, 300.0, Bg).astype(np.float32))))
    gl = [sharded.sharded_glove_step(emb, bia, inp, tgt, ops.GLOVE_REFERENCE, tx) for inp, tgt in gb]
    E, Bt = T(e0), T(b0)
    ms, ns = [torch.zeros_like(E), torch.zeros_like(Bt)], [torch.zeros_like(E), torch.zeros_like(Bt)]
    ls = [torch.zeros(V, dtype=torch.int32, device=dev) for _ in range(2)]
    for t, (inp, tgt) in enumerate(gb, 1):
        ids = inp.reshape(-1)
        ops.adam_catchup_rows([(E, ms[0], ns[0], ls[0], ids, 0)], t, LR_A)   # (one table per launch: each group's geometry)
        ops.adam_catchup_rows([(Bt, ms[1], ns[1], ls[1], ids, 0)], t, LR_A)
        loss, grow, gbias = ops.glove_fwd_bwd(E, Bt, inp, tgt, ops.GLOVE_REFERENCE)
        assert _equal(loss.reshape(-1), gl[t - 1].reshape(-1)), t
        srt, perm = ops.segment_sort(ids, V)
        ops.sparse_adam_step_lazy([E], [ms[0]], [ns[0]], [ls[0]], [0, V], srt, perm, grow, LR_A, t)
        ops.sparse_adam_step_lazy([Bt], [ms[1]], [ns[1]], [ls[1]], [0, V], srt, perm, gbias.reshape(-1, 1), LR_A, t)
    for g, P, m, n, l in ((emb, E, ms[0], ns[0], ls[0]), (bia, Bt, ms[1], ns[1], ls[1])):
        st = g.opt_state
        assert _equal(g.tables[0].local, P) and _equal(st["mu"][0], m) and _equal(st["nu"][0], n)
        assert _equal(st["last"][0], l)


# ---- world 2 and 4 over the loopback wire ------------------------------------------------------------------------------
NW = 10  # steps: Zipf tails leave rows untouched for more than 8 of them


def _world_worker(rank, port, outdir, wire_lib, world):
    dist, dev = ww._init(rank, world, port, wire_lib)
    from esrecsys_amd import ops, optim, replicated, sharded
    tx = optim.adam(LR_A, lazy=True)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    st0, pt0 = ww._towers_full()
    gbs = float(world * ww.B)

    def towers(grad_dtype=None):
        return sharded.ShardedTableGroup([sharded.RowShardedTable(T(st0[rank::world]), None, ww.V_S),
                                          sharded.RowShardedTable(T(pt0[rank::world]), None, ww.V_P)],
                                         kernels=ops, grad_dtype=grad_dtype)

    def books(g):
        s = g.adam_state()
        return [t.local.cpu().numpy() for t in g.tables] + [m.cpu().numpy() for m in s["mu"]] + \
            [v.cpu().numpy() for v in s["nu"]]

    trip = [tuple(T(a) for a in ww._batch(s, rank, zipf=True)) for s in range(NW)]
    out = {}
    g = towers()
    assert g.exchange() is not None, "the library's exchange must be under test"
    losses = [sharded.sharded_triplet_step(g, *b, ww.LAM, gbs, tx) for b in trip]
    for i, a in enumerate(books(g)):
        out["trip_%d" % i] = a
    out["steps_loss"] = np.array([float(l) for l in losses])
    for name, gd in (("helper", None), ("bf16", "bf16")):
        g = towers(gd)
        losses = sharded.sharded_train_steps("triplet", (g,), trip, regularization=ww.LAM, global_batch_size=gbs, lr=tx,
                                             plan_group=4)
        for i, a in enumerate(books(g)):
            out["%s_%d" % (name, i)] = a
        out[name + "_loss"] = np.array([float(l) for l in losses])
    # GloVe, diagonal mode, Zipf ids
    e0, b0 = ww._glove_full()
    emb = sharded.ShardedTableGroup([sharded.RowShardedTable(T(e0[rank::world]), None, ww.V_G)], kernels=ops)
    bia = sharded.ShardedTableGroup([sharded.RowShardedTable(T(b0[rank::world]), None, ww.V_G)], kernels=ops)
    for s in range(NW):
        inp, tgt = ww._glove_batch(s, rank, True)
        sharded.sharded_glove_step(emb, bia, T(inp), T(tgt), ops.GLOVE_DIAGONAL, tx)
    for i, a in enumerate(books(emb) + books(bia)):
        out["glove_%d" % i] = a
    # replicated: full tables on every rank
    rep = replicated.ReplicatedTables([T(st0), T(pt0)], [None, None], kernels=ops)
    assert rep.coll.x is not None
    for b in trip:
        replicated.replicated_triplet_step(rep, *b, ww.LAM, gbs, tx)
    s = rep.adam_state()
    for i, a in enumerate([t.cpu().numpy() for t in rep.tables] + [m.cpu().numpy() for m in s["mu"]] +
                          [v.cpu().numpy() for v in s["nu"]]):
        out["rep_%d" % i] = a
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    ww._finish(dist)


def _spawn(world):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import importlib.util
    spec = importlib.util.spec_from_file_location("build_wire", os.path.join(ROOT, "tests", "wire", "build_wire.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    wire_lib = mod.build()
    import torch.multiprocessing as mp
    os.environ.setdefault("ESR_WIRE_TIMEOUT_S", "45")
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_world_worker, args=(free_port(), d, wire_lib, world), nprocs=world, join=True)
        return [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(world)]


# the hyper-parameters as the fp32 kernels hold them: 1 - float32(0.999) is 1.3e-5 away from 0.001, and nu would be too
HP32 = {k: float(np.float32(v)) for k, v in dict(lr=LR_A, b1=0.9, b2=0.999, eps=1e-8).items()}
HP32["dtype"] = np.float64


def _dense_adam_replay_triplet(world):
    """fp64 dense optax.adam on the unsharded towers, every rank's batch of every step."""
    from oracle import optim as o_optim
    from oracle import stl_head as o_stl
    st, pt = (t.astype(np.float64) for t in ww._towers_full())
    ss, sp = o_optim.adam_init(st), o_optim.adam_init(pt)
    for step in range(NW):
        parts = [ww._batch(step, r, zipf=True) for r in range(world)]
        sid, pid, nid = (np.concatenate([p[i] for p in parts]) for i in range(3))
        _, gs, gp, gn = o_stl.triplet_loss_and_grads(st[sid], pt[pid], pt[nid], ww.LAM, world * ww.B, np.float64)
        g_s, g_p = np.zeros_like(st), np.zeros_like(pt)
        np.add.at(g_s, sid, gs)
        np.add.at(g_p, pid, gp)
        np.add.at(g_p, nid, gn)
        st, ss = o_optim.adam_update(st, g_s, ss, **HP32)
        pt, sp = o_optim.adam_update(pt, g_p, sp, **HP32)
    return [st, pt, ss["mu"], sp["mu"], ss["nu"], sp["nu"]]


def _dense_adam_replay_glove(world):
    from oracle import glove as o_glove
    from oracle import optim as o_optim
    emb, bias = (t.astype(np.float64) for t in ww._glove_full())
    se, sb = o_optim.adam_init(emb), o_optim.adam_init(bias)
    for step in range(NW):
        g_e, g_b = np.zeros_like(emb), np.zeros_like(bias)
        for r in range(world):
            inp, tgt = ww._glove_batch(step, r, True)
            _, gdot, gs = o_glove.loss_and_grads(emb, bias, inp, tgt.astype(np.float64), "diagonal", np.float64)
            ids, rows, gb = o_glove.row_grads(emb, inp, gdot, gs, np.float64)
            np.add.at(g_e, ids, rows)
            np.add.at(g_b[:, 0], ids, gb)
        emb, se = o_optim.adam_update(emb, g_e, se, **HP32)
        bias, sb = o_optim.adam_update(bias, g_b, sb, **HP32)
    return [emb, se["mu"], se["nu"], bias, sb["mu"], sb["nu"]]


def _assemble(outs, key, world):
    parts = [o[key] for o in outs]
    full = np.zeros((sum(p.shape[0] for p in parts),) + parts[0].shape[1:], parts[0].dtype)
    for r in range(world):
        full[r::world] = parts[r]
    return full


def _bf16_bound(bad, o, i, start, name):
    """bf16 gradient rows against f32 ones (the same loop): the moments they feed -- mu linearly, nu quadratically -- stay
    inside the bf16 gradient exchange test's bound, 2^-7 of the largest element.  The tables do too, but for the few
    elements whose gradient nearly cancels across ranks: Adam's step does not scale with the gradient, so the rounding of
    each rank's share may decide its sign (~1e-4 of the elements at these sizes).  Those are held to 1e-3 of the
    elements, and the rms error to 2^-6 of the rms displacement."""
    exact, half = o["helper_%d" % i], o["bf16_%d" % i]
    for j, what in ((i + 2, "mu"), (i + 4, "nu")):
        e, x = o["bf16_%d" % j], o["helper_%d" % j]
        if not 0.0 < np.abs(e - x).max() <= 2.0 ** -7 * np.abs(x).max():
            bad.append(("bf16 %s_%s" % (what, name), float(np.abs(e - x).max()), float(np.abs(x).max())))
    d, moved = half - exact, exact - start
    over = int((np.abs(d) > 2.0 ** -7 * np.abs(moved).max()).sum())
    rms = float(np.sqrt(np.mean(d * d) / np.mean(moved * moved)))
    if not (0 < np.abs(d).max() and over <= 1e-3 * d.size and rms <= 2.0 ** -6):
        bad.append(("bf16 " + name, over, d.size, rms))


def _close(bad, got, exp, what):
    """Within 1e-5 of the largest element: the fp64 replay rounds nothing, the steps round in fp32 (run sums across ranks
    in another order, fp32 gradients of the loss kernels, the long-gap closed form)."""
    err, scale = np.abs(got - exp).max(), np.abs(exp).max()
    if not err <= 1e-5 * scale:
        bad.append((what, float(err), float(scale)))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world", [2, 4])
def test_world_n_lazy_adam_matches_dense_adam_over_the_wire(world):
    outs = _spawn(world)
    bad = []
    names = ["scene", "prod", "mu_scene", "mu_prod", "nu_scene", "nu_prod"]
    exp = _dense_adam_replay_triplet(world)
    start = ww._towers_full()
    for i, name in enumerate(names):
        got = _assemble(outs, "trip_%d" % i, world)
        _close(bad, got, exp[i], name)
        # the loop helper equals the per-step calls bit for bit
        assert all(np.array_equal(o["trip_%d" % i], o["helper_%d" % i]) for o in outs), name
        if i < 2:
            for r, o in enumerate(outs):
                _bf16_bound(bad, o, i, start[i][r::world], name)
        # replicated: replicas bit-identical, and the same dense Adam
        assert all(np.array_equal(o["rep_%d" % i], outs[0]["rep_%d" % i]) for o in outs), name
        _close(bad, outs[0]["rep_%d" % i], exp[i], "replicated " + name)
    assert all(np.array_equal(o["steps_loss"], o["helper_loss"]) for o in outs)
    gexp = _dense_adam_replay_glove(world)
    for i, name in enumerate(["emb", "mu_emb", "nu_emb", "bias", "mu_bias", "nu_bias"]):
        _close(bad, _assemble(outs, "glove_%d" % i, world), gexp[i], "glove " + name)
    assert not bad, bad

"""GPU: lazy optax.adam (optim.adam(lazy=True)) against the engine's dense Adam and an fp64 replay.

Contract (include/esr_hip.h): touched rows and gaps of <= ops.ADAM_EXACT_STEPS steps are bit-identical to the dense
optimizer in p, mu and nu; a longer gap is within 1e-6 |dp| + 2 ulp(p) (p) and 1e-6 relative (mu, nu) of an fp64 replay of
the missed steps; rows with mu = nu = 0 never move."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import glove as o_glove
from oracle import optim as o_optim

pytestmark = pytest.mark.gpu
F64 = np.float64
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def N(t):
    return t.detach().cpu().numpy()


def _W():
    from esrecsys_amd import ops
    return ops.ADAM_EXACT_STEPS


def replay64(p, m, v, t0, n, lr=LR, b1=B1, b2=B2, eps=EPS):
    """n zero-gradient optax.adam steps t0 + 1 .. t0 + n in fp64 (bias corrections exact) with the engine's fp32
    hyperparameters."""
    p, m, v = (np.asarray(a, F64).copy() for a in (p, m, v))
    p0 = p.copy()
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    for t in range(t0 + 1, t0 + n + 1):
        m *= b1
        v *= b2
        p -= lr * (m / (1.0 - b1 ** t)) / (np.sqrt(v / (1.0 - b2 ** t)) + eps)
    return p, m, v, p - p0


def assert_contract(p, m, v, ref):
    rp, rm, rv, dp = ref
    p, m, v = (np.asarray(a, F64) for a in (p, m, v))
    ulp = np.spacing(np.abs(rp).astype(np.float32)).astype(F64)
    assert np.all(np.abs(p - rp) <= 1e-6 * np.abs(dp) + 2 * ulp), float(np.max(np.abs(p - rp) - 1e-6 * np.abs(dp) - 2 * ulp))
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(m - rm) <= 1e-6 * np.abs(rm) + tiny)
    assert np.all(np.abs(v - rv) <= 1e-6 * np.abs(rv) + tiny)


def _rows(dev, V, D, seed):
    """p, mu, nu of a table mid-training: row 0 never touched (mu = nu = 0), row 1 eps-dominated (tiny nu), row 2 nu
    across the regimes of the long-gap form, the rest ordinary."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(V, D, generator=g) * 0.1
    m = torch.randn(V, D, generator=g) * 1e-3
    v = torch.rand(V, D, generator=g) * 1e-6
    m[0] = 0
    v[0] = 0
    v[1] = torch.rand(D, generator=g) * 1e-21
    m[1] = torch.randn(D, generator=g) * 1e-9
    v[2] = torch.from_numpy(np.logspace(-24, -4, D)).float()
    return p.to(dev), m.to(dev), v.to(dev)


@pytest.mark.parametrize("D", [1, 3, 16, 128, 256, 512])
@pytest.mark.parametrize("t0", [1, 10, 10000])
def test_catchup_against_dense_zero_gradient_steps(dev, D, t0):
    from esrecsys_amd import ops
    W = _W()
    V = 7
    for n in (1, 2, W - 1, W, W + 1, 100, 1000, 20000):
        p, m, v = _rows(dev, V, D, seed=D * 7 + t0 + n)
        last = torch.full((V,), t0, dtype=torch.int32, device=dev)
        ids = torch.tensor([0, 1, 2, 3, 5, 3, 1, 6], dtype=torch.int32, device=dev)  # row 4 is not read
        p0, m0, v0 = N(p), N(m), N(v)
        lp, lm, lv = p.clone(), m.clone(), v.clone()
        ops.adam_catchup_rows([(lp, lm, lv, last, ids, 0)], t0 + n + 1, LR)
        torch.cuda.synchronize()
        assert N(last).tolist() == [t0 + n] * 4 + [t0] + [t0 + n] * 2
        assert np.array_equal(N(lp)[4], p0[4]) and np.array_equal(N(lm)[4], m0[4]) and np.array_equal(N(lv)[4], v0[4])
        # a row with mu = nu = 0 never moves
        assert np.array_equal(N(lp)[0], p0[0]) and not N(lm)[0].any() and not N(lv)[0].any()
        rows = [0, 1, 2, 3, 5, 6]
        if n <= W:
            dp, dm, dv = p.clone(), m.clone(), v.clone()
            zero = torch.zeros_like(p)
            for t in range(t0 + 1, t0 + n + 1):
                ops.dense_adam(dp, dm, dv, zero, LR, t)
            for a, b in ((lp, dp), (lm, dm), (lv, dv)):
                assert np.array_equal(N(a)[rows], N(b)[rows]), (n, D, t0)
        else:
            ref = replay64(p0[rows], m0[rows], v0[rows], t0, n)
            assert_contract(N(lp)[rows], N(lm)[rows], N(lv)[rows], ref)


@pytest.mark.parametrize("D", [1, 64, 256])
def test_flush_against_dense(dev, D):
    """esr_adam_flush: every row behind `step` brought up to it -- bit-exact for short gaps, the contract beyond."""
    from esrecsys_amd import ops
    W = _W()
    V, t0 = 9, 40
    p, m, v = _rows(dev, V, D, seed=D)
    gaps = [0, 1, 2, W, W + 1, 30, 40, 3, W - 1]  # row r is gaps[r] steps behind step t0 + 40
    now = t0 + 40
    last = torch.tensor([now - g for g in gaps], dtype=torch.int32, device=dev)
    p0, m0, v0 = N(p), N(m), N(v)
    ops.adam_flush(p, m, v, last, now, LR)
    torch.cuda.synchronize()
    assert (N(last) == now).all()
    for r, g in enumerate(gaps):
        if g <= W:
            dp, dm, dv = (torch.from_numpy(a[r:r + 1].copy()).to(dev) for a in (p0, m0, v0))
            for t in range(now - g + 1, now + 1):
                ops.dense_adam(dp, dm, dv, torch.zeros_like(dp), LR, t)
            assert np.array_equal(N(p)[r], N(dp)[0]) and np.array_equal(N(m)[r], N(dm)[0]) and np.array_equal(N(v)[r], N(dv)[0])
        else:
            assert_contract(N(p)[r], N(m)[r], N(v)[r], replay64(p0[r], m0[r], v0[r], now - g, g))


def _zipf_ids(rng, V, n, a=1.3):
    return ((rng.zipf(a, n) - 1) % V).astype(np.int32)


@pytest.mark.parametrize("D,ntables", [(1, 1), (64, 1), (128, 2), (256, 1)])
def test_sparse_step_equals_dense_step(dev, D, ntables):
    """One lazy step on current tables against to_dense + dense_adam on the same gradient rows: Zipf ids with runs longer
    than one 32-position chunk (segment_long_kernel), two tables through virtual rows."""
    from esrecsys_amd import ops
    rng = np.random.default_rng(D + ntables)
    Vt = [3000, 2000][:ntables]
    n = 20000
    step = 12
    tabs = [_rows(dev, V, D, seed=V + D) for V in Vt]
    offs = [0]
    for V in Vt:
        offs.append(offs[-1] + V)
    vids = np.concatenate([offs[k] + _zipf_ids(rng, Vt[k], n // ntables) for k in range(ntables)])
    rng.shuffle(vids)
    vids_t = torch.from_numpy(vids).to(dev)
    sorted_vids, perm = ops.segment_sort(vids_t, offs[-1])
    counts = np.bincount(vids, minlength=offs[-1])
    assert counts.max() > 64  # a run spanning several chunks
    grad = (torch.randn(vids.size, D, generator=torch.Generator().manual_seed(3)) * 1e-2).to(dev)
    lasts = [torch.full((V,), step - 1, dtype=torch.int32, device=dev) for V in Vt]
    dense = [tuple(t.clone() for t in tab) for tab in tabs]
    g_all = ops.rows_to_dense(offs[-1], D, sorted_vids, perm, grad.clone())
    for k, (p, m, v) in enumerate(dense):
        ops.dense_adam(p, m, v, g_all[offs[k]:offs[k + 1]].contiguous(), LR, step)
    before = [tuple(N(t) for t in tab) for tab in tabs]
    ops.sparse_adam_step_lazy([t[0] for t in tabs], [t[1] for t in tabs], [t[2] for t in tabs], lasts, offs, sorted_vids,
                              perm, grad.clone(), LR, step)
    torch.cuda.synchronize()
    for k in range(ntables):
        touched = counts[offs[k]:offs[k + 1]] > 0
        assert (N(lasts[k])[touched] == step).all() and (N(lasts[k])[~touched] == step - 1).all()
        for a, b, b0 in zip(tabs[k], dense[k], before[k]):
            assert np.array_equal(N(a)[touched], N(b)[touched])
            assert np.array_equal(N(a)[~touched], b0[~touched])  # untouched rows: not one byte
        # the untouched rows owe one zero-gradient step: a flush settles it, bit for bit
        ops.adam_flush(*tabs[k], lasts[k], step, LR)
        for a, b in zip(tabs[k], dense[k]):
            assert np.array_equal(N(a), N(b))


# ---- GloVe -------------------------------------------------------------------------------------------------------------

def _glove_state(dev, V, D, tx, seed=1701):
    from esrecsys_amd import TrainState
    from esrecsys_amd.wikipedia.models import Glove
    model = Glove(num_embeddings=V, features=D, device=dev)
    params = model.init(seed, None)["params"]
    g = torch.Generator().manual_seed(seed + 1)
    params["_bias"]["embedding"].copy_((torch.randn((V, 1), generator=g) * 0.05).to(dev))
    return model, TrainState.create(apply_fn=model.apply, params=params, tx=tx)


def _clone_state(dev, V, D, tx, seed=1701):
    return _glove_state(dev, V, D, tx, seed)[1]


def _tree_arrays(state):
    p = state.params
    mu, nu = state.opt_state["mu"], state.opt_state["nu"]
    out = {}
    for k in p:
        out[k] = (N(p[k]["embedding"]), N(mu[k]["embedding"]), N(nu[k]["embedding"]))
    return out


def _glove_batches(rng, V, B, steps, period):
    """Step s reads the rows r with r % period == s % period (and only those): every row is caught up over
    period - 1 missed steps each time it is read -- within the exact window when period <= ADAM_EXACT_STEPS + 1."""
    out = []
    for s in range(steps):
        block = np.arange(s % period, V, period)
        x = rng.choice(block, (2, B)).astype(np.int32)
        x[0, :block.size] = block
        out.append((x, rng.uniform(0.5, 300, B).astype(np.float32)))
    return out


def test_glove_short_gaps_bit_equal_to_dense(dev):
    from esrecsys_amd import optim
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    V, D, B = 64, 32, 128
    batches = _glove_batches(np.random.default_rng(1), V, B, 50, period=_W() + 1)
    lazy = _clone_state(dev, V, D, optim.adam(LR, lazy=True))
    dense = _clone_state(dev, V, D, optim.adam(LR))
    for x, y in batches:
        g, l_lazy = apply_model(lazy, x, y)
        assert all(type(g[k]["embedding"]).__name__ == "RowGrads" for k in g)  # row-sparse: no to_dense
        lazy = update_model(lazy, g)
        g, l_dense = apply_model(dense, x, y)
        dense = update_model(dense, g)
        assert float(l_lazy) == float(l_dense)
    assert lazy.opt_state["count"] == dense.opt_state["count"] == 50
    a, b = _tree_arrays(lazy), _tree_arrays(dense)
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k


def test_glove_train_epoch_short_gaps_bit_equal(dev):
    from esrecsys_amd import optim
    from esrecsys_amd.wikipedia.train_cooccurence import train_epoch
    V, D, B = 64, 16, 96
    batches = _glove_batches(np.random.default_rng(2), V, B, 30, period=4)
    lazy = _clone_state(dev, V, D, optim.adam(LR, lazy=True))
    dense = _clone_state(dev, V, D, optim.adam(LR))
    lazy, l1 = train_epoch(lazy, 30, iter(batches))
    dense, l2 = train_epoch(dense, 30, iter(batches))
    assert float(l1) == float(l2)
    a, b = _tree_arrays(lazy), _tree_arrays(dense)
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x, y), k
    assert lazy.opt_state["count"] == dense.opt_state["count"] == 30


def test_glove_long_gaps_within_contract_of_dense(dev):
    """The reference's vocabulary (V = 465 537) with Zipf ids over 200 steps: most rows go hundreds of steps unread."""
    from esrecsys_amd import optim
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    V, D, B = 465537, 256, 2048
    rng = np.random.default_rng(3)
    lazy = _clone_state(dev, V, D, optim.adam(LR, lazy=True))
    dense = _clone_state(dev, V, D, optim.adam(LR))
    p0 = N(dense.params["_token_embedding"]["embedding"]).astype(F64)
    for _ in range(200):
        x = _zipf_ids(rng, V, 2 * B, 1.2).reshape(2, B)
        y = rng.uniform(0.5, 300, B).astype(np.float32)
        g, _ = apply_model(lazy, x, y)
        lazy = update_model(lazy, g)
        g, _ = apply_model(dense, x, y)
        dense = update_model(dense, g)
    last = lazy.opt_state["_lazy"]["last"][("_token_embedding", "embedding")]
    assert int((last < 200).sum()) > 0  # rows really were left behind
    a, b = _tree_arrays(lazy), _tree_arrays(dense)
    assert (N(last) == 200).all()  # (state.params flushed)
    pe, pd = a["_token_embedding"][0].astype(F64), b["_token_embedding"][0].astype(F64)
    # (the dense path rounds p once per step, ~sqrt(200) ulp of drift on rows left alone; the lazy one once per gap)
    assert rel_err(pe - p0, pd - p0) <= 1e-3
    assert rel_err(pe, pd) <= 1e-5
    for k in a:
        for x, y in zip(a[k][1:], b[k][1:]):
            assert rel_err(x, y) <= 1e-4


def test_glove_lazy_adam_against_fp64_oracle(dev):
    """The thresholds tests/test_gpu_api.py holds the dense path to, over enough steps that some gaps exceed the window."""
    from esrecsys_amd import optim
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    V, D, B = 300, 16, 64
    _, state = _glove_state(dev, V, D, optim.adam(LR, lazy=True))
    emb = N(state.params["_token_embedding"]["embedding"]).astype(F64)
    bias = N(state.params["_bias"]["embedding"]).astype(F64)
    emb0 = emb.copy()
    s_emb, s_bias = o_optim.adam_init(emb), o_optim.adam_init(bias)
    rng = np.random.default_rng(6)
    for step in range(16):
        inputs = rng.integers(0, V, (2, B)).astype(np.int32)
        target = rng.uniform(0.01, 300, B).astype(np.float32)
        grads, loss = apply_model(state, inputs, target)
        state = update_model(state, grads)
        eg, el = o_glove.dense_grads(emb, bias, inputs, target, "reference", F64)
        emb, s_emb = o_optim.adam_update(emb, eg["_token_embedding"]["embedding"], s_emb, LR, dtype=F64)
        bias, s_bias = o_optim.adam_update(bias, eg["_bias"]["embedding"], s_bias, LR, dtype=F64)
    got = N(state.params["_token_embedding"]["embedding"]).astype(F64)
    assert rel_err(got - emb0, emb - emb0) <= 1e-3
    assert rel_err(got, emb) <= 1e-6
    assert state.opt_state["count"] == 16


# ---- Shop-The-Look -----------------------------------------------------------------------------------------------------

def _stl_state(dev, Vs, Vp, D, tx, seed=0):
    from esrecsys_amd import TrainState
    from esrecsys_amd.pinterest.models import STLModel
    stl = STLModel(output_size=D, num_scenes=Vs, num_products=Vp, device=dev)
    params = stl.init(seed, None, None, None)
    for k in ("scene_tower", "product_tower"):
        params["params"][k]["embedding"].mul_(1.4)
    return TrainState.create(apply_fn=stl.apply, params=params, tx=tx)


def _stl_arrays(state):
    out = []
    for k in ("scene_tower", "product_tower"):
        out += [N(state.params["params"][k]["embedding"]), N(state.opt_state["mu"]["params"][k]["embedding"]),
                N(state.opt_state["nu"]["params"][k]["embedding"])]
    return out


@pytest.mark.parametrize("inbatch", [False, True])
def test_stl_short_gaps_bit_equal_to_dense(dev, inbatch):
    from esrecsys_amd import optim
    from esrecsys_amd.pinterest.train_shop_the_look import train_step
    Vs, Vp, D, B = 64, 96, 128, 256
    rng = np.random.default_rng(4)
    lazy = _stl_state(dev, Vs, Vp, D, optim.adam(LR, lazy=True))
    dense = _stl_state(dev, Vs, Vp, D, optim.adam(LR))
    period = 4  # step s reads the rows r with r % 4 == s % 4: gaps of 3 steps
    for s in range(50):
        bs, bp = np.arange(s % period, Vs, period), np.arange(s % period, Vp, period)
        sc = rng.choice(bs, B).astype(np.int32)
        sc[:bs.size] = bs
        po = rng.choice(bp, B).astype(np.int32)
        po[:bp.size] = bp
        ne = None if inbatch else rng.choice(bp, B).astype(np.int32)
        lazy, l1 = train_step(lazy, sc, po, ne, 0.1, B, precision="f32")
        dense, l2 = train_step(dense, sc, po, ne, 0.1, B, precision="f32")
        assert float(l1) == float(l2)
    assert lazy.opt_state["count"] == dense.opt_state["count"] == 50
    for x, y in zip(_stl_arrays(lazy), _stl_arrays(dense)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("inbatch", [False, True])
def test_stl_train_steps_long_gaps_within_contract(dev, inbatch):
    from esrecsys_amd import optim
    from esrecsys_amd.pinterest.train_shop_the_look import train_steps
    Vs, Vp, D, B = 20000, 50000, 128, 1024
    rng = np.random.default_rng(5)
    batches = [(_zipf_ids(rng, Vs, B), _zipf_ids(rng, Vp, B), None if inbatch else _zipf_ids(rng, Vp, B))
               for _ in range(60)]
    lazy = _stl_state(dev, Vs, Vp, D, optim.adam(LR, lazy=True))
    dense = _stl_state(dev, Vs, Vp, D, optim.adam(LR))
    p0 = [x.astype(F64) for x in _stl_arrays(dense)[::3]]
    lazy, _ = train_steps(lazy, iter(batches), 60, regularization=0.1, batch_size=B, precision="f32")
    dense, _ = train_steps(dense, iter(batches), 60, regularization=0.1, batch_size=B, precision="f32")
    a, b = _stl_arrays(lazy), _stl_arrays(dense)
    for k in range(2):
        pe, pd = a[3 * k].astype(F64), b[3 * k].astype(F64)
        assert rel_err(pe - p0[k], pd - p0[k]) <= 1e-3
        assert rel_err(pe, pd) <= 1e-5
        assert rel_err(a[3 * k + 1], b[3 * k + 1]) <= 1e-4 and rel_err(a[3 * k + 2], b[3 * k + 2]) <= 1e-4


# ---- laziness, flush, dense steps, checkpoints ------------------------------------------------------------------------

def test_untouched_rows_are_not_touched_until_params_flushes(dev):
    from esrecsys_amd import optim
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    V, D, B = 1000, 32, 64
    rng = np.random.default_rng(7)
    lazy = _clone_state(dev, V, D, optim.adam(LR, lazy=True))
    dense = _clone_state(dev, V, D, optim.adam(LR))
    batches = [(rng.integers(0, 200, (2, B)).astype(np.int32), rng.uniform(0.5, 300, B).astype(np.float32))
               for _ in range(5)]
    for x, y in batches[:4]:
        lazy = update_model(lazy, apply_model(lazy, x, y)[0])
        dense = update_model(dense, apply_model(dense, x, y)[0])
    raw = lazy.raw_params["_token_embedding"]["embedding"]
    mu = lazy.opt_state["mu"]["_token_embedding"]["embedding"]
    before = N(raw).copy(), N(mu).copy()
    x, y = batches[4]
    lazy = update_model(lazy, apply_model(lazy, x, y)[0])
    dense = update_model(dense, apply_model(dense, x, y)[0])
    last = N(lazy.opt_state["_lazy"]["last"][("_token_embedding", "embedding")])
    read = np.zeros(V, bool)
    read[x.reshape(-1)] = True
    assert (last[read] == 5).all() and (last[~read] < 5).all()
    assert np.array_equal(N(raw)[~read], before[0][~read]) and np.array_equal(N(mu)[~read], before[1][~read])
    # rows 200.. were never read: mu = nu = 0, they never move at all
    assert np.array_equal(N(raw)[200:], before[0][200:])
    _ = lazy.params  # flush
    assert (N(lazy.opt_state["_lazy"]["last"][("_token_embedding", "embedding")]) == 5).all()
    a, b = _tree_arrays(lazy), _tree_arrays(dense)
    for k in a:
        for u, w in zip(a[k], b[k]):
            assert np.array_equal(u, w)


def test_dense_step_after_lazy_steps_flushes_first(dev):
    from esrecsys_amd import optim
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    V, D, B = 500, 16, 64
    rng = np.random.default_rng(8)
    lazy = _clone_state(dev, V, D, optim.adam(LR, lazy=True))
    dense = _clone_state(dev, V, D, optim.adam(LR))
    for _ in range(5):
        x, y = rng.integers(0, 100, (2, B)).astype(np.int32), rng.uniform(0.5, 300, B).astype(np.float32)
        lazy = update_model(lazy, apply_model(lazy, x, y)[0])
        dense = update_model(dense, apply_model(dense, x, y)[0])
    x, y = rng.integers(0, 100, (2, B)).astype(np.int32), rng.uniform(0.5, 300, B).astype(np.float32)
    g, _ = apply_model(dense, x, y)
    gd = {k: {"embedding": g[k]["embedding"]} for k in g}  # dense gradient tensors (dense Adam's apply_model)
    assert all(isinstance(gd[k]["embedding"], torch.Tensor) for k in gd)
    gl = {k: {"embedding": gd[k]["embedding"].clone()} for k in gd}
    dense = update_model(dense, gd)
    lazy = update_model(lazy, gl)
    assert lazy.opt_state["count"] == 6
    assert (N(lazy.opt_state["_lazy"]["last"][("_token_embedding", "embedding")]) == 6).all()
    a, b = _tree_arrays(lazy), _tree_arrays(dense)
    for k in a:
        for u, w in zip(a[k], b[k]):
            assert np.array_equal(u, w)


def test_checkpoint_bytes_and_resume(dev):
    from esrecsys_amd import checkpoint, optim
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    V, D, B = 64, 16, 96
    batches = _glove_batches(np.random.default_rng(9), V, B, 20, period=3)
    lazy = _clone_state(dev, V, D, optim.adam(LR, lazy=True))
    dense = _clone_state(dev, V, D, optim.adam(LR))
    for x, y in batches[:10]:
        lazy = update_model(lazy, apply_model(lazy, x, y)[0])
        dense = update_model(dense, apply_model(dense, x, y)[0])
    blob = checkpoint.to_bytes(lazy)
    assert blob == checkpoint.to_bytes(dense)
    fresh = _clone_state(dev, V, D, optim.adam(LR, lazy=True), seed=5)
    resumed = checkpoint.from_bytes(fresh, blob)
    assert resumed.opt_state["count"] == 10
    for x, y in batches[10:]:
        resumed = update_model(resumed, apply_model(resumed, x, y)[0])
        dense = update_model(dense, apply_model(dense, x, y)[0])
        a, b = _tree_arrays(resumed), _tree_arrays(dense)
        for k in a:
            for u, w in zip(a[k], b[k]):
                assert np.array_equal(u, w)

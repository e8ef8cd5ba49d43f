"""GPU: the epoch loops' long-run LAUNCHES, counted by the library's own launch counters (esr_kernel_timing).  A long-run
hint that gets lost on the host (loop_plan: generations, stale words, events) leaves tables and losses bit-identical and
only adds a launch per step, so the bit-for-bit loop tests cannot see it: these pin the counts.  Every pinned count was
first read off the loops as they were before loop_plan existed, with this test body."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, B, D, HOT_STEP = 20, 64, 16, 4   # lists of 64; batch 4 sits in the middle of the first full group in every loop


def _launches(fn):
    """{kernel name: launches} of the library during fn()"""
    from esrecsys_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.esr_kernel_timing(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.esr_kernel_timing_read(buf, len(buf))
    finally:
        lib.esr_kernel_timing(0)
    return {line.split("\t")[0]: int(line.split("\t")[1]) for line in buf.value.decode().split("\n") if line}


def _distinct(rng, V, n, hot):
    """n distinct ids below V -- no run of an occurrence list outgrows a 32-position chunk; hot: 40 of them are id 7"""
    ids = rng.permutation(V)[:n].astype(np.int32)
    if hot:
        ids[:40] = 7
    return ids


# ---- Shop-The-Look -----------------------------------------------------------------------------------------------------
VS, VP = 3000, 5000


def _stl_state(dev):
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.pinterest.models import STLModel
    g = torch.Generator(device=dev).manual_seed(3)
    params = {"params": {"scene_tower": {"embedding": torch.randn((VS, D), generator=g, device=dev) * D ** -0.5},
                         "product_tower": {"embedding": torch.randn((VP, D), generator=g, device=dev) * D ** -0.5}}}
    model = STLModel(output_size=D, num_scenes=VS, num_products=VP, device=dev)
    return TrainState.create(apply_fn=model.apply, params=params, tx=optim.sparse_adagrad(0.05))


def _stl_batches(dev, hot, inbatch=False):
    rng = np.random.default_rng(17)
    out = []
    for k in range(STEPS):
        scene = _distinct(rng, VS, B, hot and k == HOT_STEP)
        prod = _distinct(rng, VP, 2 * B, False)    # pos and neg share the product tower: distinct across both
        out.append((torch.from_numpy(scene).to(dev), torch.from_numpy(prod[:B]).to(dev),
                    None if inbatch else torch.from_numpy(prod[B:]).to(dev)))
    return out


def _stl_result(state, losses):
    p, a = state.params["params"], state.opt_state["sum_of_squares"]["params"]
    return [losses] + [t[k]["embedding"] for t in (p, a) for k in ("scene_tower", "product_tower")]


def _stl_stepwise(dev, batches):
    from esrecsys_amd.pinterest.train_shop_the_look import train_step
    state, losses = _stl_state(dev), []
    for scene, pos, neg in batches:
        state, loss = train_step(state, scene, pos, neg, 0.1, float(B), scale=6.0)
        losses.append(loss.clone())
    return _stl_result(state, torch.stack(losses))


def _run_train_steps(dev, batches):
    from esrecsys_amd.pinterest.train_shop_the_look import train_steps
    out = {}

    def run():
        out["r"] = _stl_result(*train_steps(_stl_state(dev), iter(batches), STEPS, 0.1, float(B), scale=6.0))
    return _launches(run), out["r"]


def _run_presorted(dev, batches):
    from esrecsys_amd.pinterest.train_shop_the_look import presorted, train_step
    out = {}

    def run():
        state, losses = _stl_state(dev), []
        for scene, pos, neg in presorted(state, iter(batches)):
            state, loss = train_step(state, scene, pos, neg, 0.1, float(B))
            losses.append(loss.clone())
        out["r"] = _stl_result(state, torch.stack(losses))
    return _launches(run), out["r"]


def _same(got, want):
    return all(torch.equal(x, y) for x, y in zip(got, want))


# steps issued outside a planned group: train_steps sends the first step out alone (it plans in line and nobody tells it
# whether a run is long); presorted() plans every batch of 8 + 8 + 4 with its group
@pytest.mark.parametrize("loop,ungrouped", [(_run_train_steps, 1), (_run_presorted, 0)])
def test_triplet_loops_make_the_long_run_launch_only_where_a_run_is_long(dev, loop, ungrouped):
    counts, _ = loop(dev, _stl_batches(dev, False))
    print("distinct:", counts)
    assert counts.get("triplet_direct_kernel", 0) == STEPS
    assert counts.get("triplet_direct_long_kernel", 0) == ungrouped
    batches = _stl_batches(dev, True)
    counts, got = loop(dev, batches)
    print("one hot batch:", counts)
    assert counts.get("triplet_direct_kernel", 0) == STEPS
    assert counts.get("triplet_direct_long_kernel", 0) == ungrouped + 1
    assert _same(got, _stl_stepwise(dev, batches))


@pytest.mark.parametrize("loop", [_run_train_steps, _run_presorted])
def test_triplet_loops_without_the_hint_wait_compute_the_same(dev, loop, monkeypatch):
    """ESR_STL_HINT_WAIT=0: hints that have not arrived may add launches, never change a bit"""
    import esrecsys_amd.pinterest.train_shop_the_look as stl
    batches = _stl_batches(dev, True)
    _, want = loop(dev, batches)
    monkeypatch.setattr(stl, "_HINT_WAIT", False)
    _, got = loop(dev, batches)
    assert _same(got, want)


def test_inbatch_loop_makes_the_long_run_launches_only_for_a_group_with_a_long_run(dev):
    """In-batch groups (1, 2, 4, 8, 5 steps) are screened as a whole: the first step goes out alone and unscreened and
    makes the launches of an unhinted step, a screened group makes them only when one of its lists has a long run."""
    from esrecsys_amd.pinterest.train_shop_the_look import train_step
    batches = _stl_batches(dev, False, inbatch=True)
    state = _stl_state(dev)
    per_step = _launches(lambda: train_step(state, batches[0][0], batches[0][1], None, 0.1, float(B), scale=6.0)) \
        .get("segment_long_kernel", 0)
    assert per_step > 0
    counts, _ = _run_train_steps(dev, batches)
    print("unhinted step:", per_step, "distinct:", counts)
    assert counts.get("segment_long_kernel", 0) == per_step
    batches = _stl_batches(dev, True, inbatch=True)      # batch 4 belongs to the group of four (steps 3 .. 6)
    counts, got = _run_train_steps(dev, batches)
    print("one hot batch:", counts)
    assert counts.get("segment_long_kernel", 0) == per_step * (1 + 4)
    assert _same(got, _stl_stepwise(dev, batches))


# ---- GloVe -------------------------------------------------------------------------------------------------------------
V = 4000


def _glove_state(dev):
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.wikipedia.models import Glove
    model = Glove(num_embeddings=V, features=D, loss_mode="reference", device=dev)
    return TrainState.create(apply_fn=model.apply, params=model.init(5, None)["params"], tx=optim.sparse_adagrad(0.05))


def _glove_batches(dev, hot):
    rng = np.random.default_rng(23)
    return [(torch.from_numpy(_distinct(rng, V, 2 * B, hot and k == HOT_STEP).reshape(2, B)).to(dev),
             torch.from_numpy(rng.uniform(0.1, 300.0, B).astype(np.float32)).to(dev)) for k in range(STEPS)]


def _run_train_epoch(dev, batches):
    import esrecsys_amd.wikipedia.train_cooccurence as tc
    out = {}

    def run():
        losses = []
        state, _ = tc.train_epoch(_glove_state(dev), STEPS, iter(batches), losses_out=losses)
        out["r"] = [losses[0], state.params["_token_embedding"]["embedding"], state.params["_bias"]["embedding"],
                    state.opt_state["sum_of_squares"]["_token_embedding"]["embedding"]]
    return _launches(run), out["r"]


def test_glove_epoch_makes_the_long_run_launch_only_where_a_run_is_long(dev, monkeypatch):
    """train_epoch sends the first step out alone (no plan, no hint: it makes the launch), then groups of 8 + 8 + 3"""
    import esrecsys_amd.wikipedia.train_cooccurence as tc
    counts, _ = _run_train_epoch(dev, _glove_batches(dev, False))
    print("distinct:", counts)
    assert counts.get("glove_step_kernel", 0) == STEPS
    assert counts.get("glove_step_long_kernel", 0) == 1
    batches = _glove_batches(dev, True)
    counts, got = _run_train_epoch(dev, batches)
    print("one hot batch:", counts)
    assert counts.get("glove_step_kernel", 0) == STEPS
    assert counts.get("glove_step_long_kernel", 0) == 2
    monkeypatch.setattr(tc, "_HINT_WAIT", False)     # may add launches, never changes a bit
    _, unwaited = _run_train_epoch(dev, batches)
    assert _same(unwaited, got)
    monkeypatch.setattr(tc, "_SORT_BATCH", 1)        # every step sorts and plans its own list in line
    monkeypatch.setattr(tc, "_PRESORT", False)
    _, stepwise = _run_train_epoch(dev, batches)
    assert _same(stepwise, got)

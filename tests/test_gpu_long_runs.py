"""GPU: one hot row per batch, its run cut into a prescribed number of partial sums -- the long-run combination
(combine_long_runs in esr_segment.h) as the stamped triplet step and the GloVe one-pass step use it.

A run of equal sorted ids that outgrows its head chunk is summed chunk by chunk; a second kernel adds the K + 1 partial
sums: row group g of NG per workgroup takes partials g, g + NG, ... four at a time, the group sums are added in group
order.  The ladder of K + 1 puts a case on each side of every turn of that loop: 2, NG - 1, NG, NG + 1 (groups without
a partial / with one / the first group with two), 4 NG - 1, 4 NG, 4 NG + 1 (the four-in-flight round just not taken /
taken / taken with a tail), and 258 (more than 256 continuation chunks: their count needs a second pass), with the
run's head on the first and on the last position of a chunk, at D = 128 and D = 6.

* The stamped triplet step (chunks of 8, NG = 32 at both widths): cases of tests/_triplet_step_ref.py ("hot-P*-a*":
  scene id 1 has exactly that run, product id 1 the same length at the other alignment), against the fp64 oracle with
  the oracle test's own comparison and bound.  make_case asserts the margin and norm-gap conditions before any GPU work;
  tests/test_triplet_step_ref.py checks them for every spec on the CPU.
* The GloVe step (chunks of 32; NG = 8 at D = 128, 32 at D = 6): against the two-call path, the comparison and
  tolerances of test_fused_step_equals_two_call_path.

The segment engine has the same ladder in tests/test_gpu_segment_update.py.
"""
import numpy as np
import pytest

import _triplet_step_ref as R
from test_gpu_glove_step import _assert_same_tables, _make_state
from test_gpu_triplet_step_oracle import _one_step

pytestmark = pytest.mark.gpu


# ---- the stamped triplet step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", R.RUN_WIDTHS)
@pytest.mark.parametrize("case", R.HOT_CASES)
def test_stamped_triplet_step_hot_row(dev, monkeypatch, case, D):
    c = R.make_case("%s-D%d" % (case, D))
    partials, align = (int(x[1:]) for x in case.split("-")[1:])
    srt = np.sort(np.concatenate([c.sid.astype(np.int64), c.Vs + c.pid.astype(np.int64), c.Vs + c.nid.astype(np.int64)]))
    assert R.hot_partials(srt, 1, R.HOT_CHUNK) == (partials, align)      # the case is what its name says
    other = R.hot_partials(srt, c.Vs + 1, R.HOT_CHUNK)                   # the product run: the other alignment
    assert other[1] == (R.HOT_ALIGN[1] if align == R.HOT_ALIGN[0] else R.HOT_ALIGN[0]) and partials - 1 <= other[0] <= partials
    _one_step(dev, monkeypatch, "%s-D%d" % (case, D), "f32", "stamped")


# ---- the GloVe step ----------------------------------------------------------------------------------------------------
GLOVE_CHUNK = 32
GLOVE_GROUPS = {128: 8, 6: 32}  # row groups per workgroup (row_geom: 32 lanes per row at D = 128, 8 at D = 6)


def _glove_ladder(D):
    ng = GLOVE_GROUPS[D]
    return [2, ng - 1, ng, ng + 1, 4 * ng - 1, 4 * ng, 4 * ng + 1, 258]


def _glove_hot_inputs(partials, align, rng):
    """int32 [2, B]: token 1 occurs L times in the first row (L cut into `partials` partial sums), token 0 `align` times
    (it sorts in front of the run), every other token once.  Returns (inputs, V)."""
    L = R.hot_run_length(partials, align, GLOVE_CHUNK)
    B = L + align + 40
    V = 2 * B + 2
    rest = 2 + rng.permutation(V - 2)[:2 * B - L - align]
    first = np.concatenate([np.full(L, 1), np.zeros(align, np.int64), rest[:B - L - align]])
    rng.shuffle(first)
    inputs = np.stack([first, rest[B - L - align:]]).astype(np.int32)
    assert R.hot_partials(np.sort(inputs.reshape(-1)), 1, GLOVE_CHUNK) == (partials, align)
    return inputs, V


@pytest.mark.parametrize("mode", ["reference", "diagonal"])
@pytest.mark.parametrize("align", [0, GLOVE_CHUNK - 1])
@pytest.mark.parametrize("D,partials", [(D, p) for D in (128, 6) for p in _glove_ladder(D)])
def test_glove_step_hot_row_equals_two_call_path(dev, mode, D, partials, align):
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, fused_step_available, train_step, update_model
    rng = np.random.default_rng([D, partials, align])
    inputs, V = _glove_hot_inputs(partials, align, rng)
    B = inputs.shape[1]
    a, b = _make_state(V, D, mode, dev), _make_state(V, D, mode, dev)
    assert fused_step_available(a)
    for step in range(3):  # (as there: after an odd number of steps the batch's rows live in the second buffer)
        target = np.exp(rng.uniform(np.log(0.1), np.log(1000.0), B)).astype(np.float32)
        a, la = train_step(a, inputs, target)
        grads, lb = apply_model(b, inputs, target)
        b = update_model(b, grads)
        assert abs(float(la) - float(lb)) <= 2e-6 * abs(float(lb)), (step, float(la), float(lb))
    _assert_same_tables(a, b, 3)

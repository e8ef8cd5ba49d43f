"""GPU: the batched retrieval top-k (esr_retrieve_topk / esr_retrieve_topk_prepared, ops.retrieve_topk) across its chunk
plan -- esr_retrieve.hip retrieve_plan, which sizes the per-query running list from the number of queries:
  first  = min(N, max(8192, 16 k))                the dense first chunk
  chunk  = 2^29 / nq (f16r) or 2^28 / nq, rounded down to 128, at most 65 536 (ESR_RETRIEVE_LIST_LOG2 /
           ESR_RETRIEVE_CHUNK_CAP: measuring hooks that shrink it)
  ppitch = max(k, mark) + chunk, mark = max(3 k, 1536); f16r: at least `first` (its first select copies a whole band)
test_gpu_retrieve.py keeps nq <= 8192, where chunk is always the 65 536 cap; these tests reach the regimes where the later
chunk is short: ppitch below `first` without the f16r floor (many queries, or the hooks at a few), and hundreds of chunks
per call (append, lazy compaction, exact-row re-score chunk after chunk), plus the chunk boundaries of the default plan.

Bar: grid-valued inputs (every product and sum exact in every mode, so ties are real) -> indices and scores bit-exact
against oracle/topk.py; real-valued inputs -> the fp64 ranking outside near-ties (test_gpu_retrieve._f16r_vs_exact's rule)."""
import functools

import numpy as np
import pytest
import torch

from oracle import topk as o_topk
from test_gpu_retrieve import F64, N, T, _grid

pytestmark = pytest.mark.gpu
MODES = ["exact", "f16x2", "bf16", "f16r"]     # "exact" = bf16x3


def _first(N_, k):
    return min(N_, max(8192, 16 * k))


def _all_modes_bit_exact(dev, q, c, k, es, ei, base=0, step=1):
    """every mode, plain and on a prepared corpus: indices and scores bit for bit the oracle's"""
    from esrecsys_amd import ops
    qd, cd = T(q, dev), T(c, dev)
    want_i = (base + step * ei.astype(np.int64)).astype(np.int32)
    want_s = es.astype(np.float32)
    for mode in MODES:
        prep = ops.retrieve_prepare(cd, mode=mode)
        for prepared in (None, prep):
            s, i = ops.retrieve_topk(qd, cd, k, mode=mode, index_base=base, index_step=step, prepared=prepared)
            what = (mode, "prepared" if prepared is not None else "plain")
            assert np.array_equal(N(i), want_i), what
            assert np.array_equal(N(s), want_s), what


# ---- a. many queries, the real plan (no hooks) ----------------------------------------------------------------------
def _vs_fp64_in_blocks(q, c, k, s, i, block=4096):
    """the fp64 ranking, a block of query rows at a time on the device: per row the true k-th and (k+1)-th best scores,
    the lowest true score among the reported indices; the largest |reported - true score of its index| and
    |reported - true k best, in order|; the largest |true score| (the yardstick)"""
    nq = q.shape[0]
    kth = torch.empty(nq, dtype=torch.float64, device=q.device)
    nxt, worst = torch.empty_like(kth), torch.empty_like(kth)
    err_own = err_rank = scale = 0.0
    cd = c.double()
    for r0 in range(0, nq, block):
        r1 = min(nq, r0 + block)
        full = q[r0:r1].double() @ cd.T
        top = torch.topk(full, k + 1, dim=1).values
        kth[r0:r1], nxt[r0:r1] = top[:, k - 1], top[:, k]
        picked = full.gather(1, i[r0:r1].long())
        worst[r0:r1] = picked.min(dim=1).values
        err_own = max(err_own, float((picked - s[r0:r1].double()).abs().max()))
        err_rank = max(err_rank, float((top[:, :k] - s[r0:r1].double()).abs().max()))
        scale = max(scale, float(full.abs().max()))
        del full, top, picked
    return kth, nxt, worst, err_own, err_rank, scale


@pytest.mark.parametrize("nq,k", [(100_000, 500), (65_536, 1024)])
def test_retrieve_f16r_many_queries_lists_shorter_than_the_first_chunk(dev, nq, k):
    """Regime: f16r at many queries, default plan.  N = 40 000, D = 128: nq = 100 000, k = 500 -> first 8192, chunk 5248
    (7 chunks), mark + chunk = 6784 < first; nq = 65 536, k = 1024 (sharded_find_top_k's all-gathered batch at world 8)
    -> first 16 384, chunk 8192 (4 chunks), mark + chunk = 11 264 < first.  Every 97th query and the last are zero (every
    score ties: the first select's band is the whole first chunk), and a few queries face 7 000 identical candidate rows
    inside the first chunk that score above everything else (a band of 7 000).  Without a list of `first` records those
    rows' bands ran into the next query's list.  Every row against the fp64 ranking and against the bf16x3 (exact) mode's
    index set outside near-ties -- the zero rows' neighbours (the victims), the last row and the rest alike; zero rows
    return 0..k-1 (ties -> lower index); the prepared-corpus call equals the plain one bit for bit."""
    from esrecsys_amd import ops
    Nc, D = 40_000, 128
    g = torch.Generator(device=dev).manual_seed(nq + k)
    q = torch.randn((nq, D), generator=g, device=dev) * D ** -0.5
    c = torch.randn((Nc, D), generator=g, device=dev) * D ** -0.5
    u = torch.randn(D, generator=g, device=dev)
    u /= u.norm()
    hot = torch.randperm(8192, generator=g, device=dev)[:7000]
    c[hot] = 1.5 * u                                   # 7 000 identical rows, all inside the first chunk
    aligned = torch.tensor([1, 2, 12_345, nq - 2], device=dev)
    q[aligned] = u                                     # (none of them a multiple of 97)
    zero = torch.cat([torch.arange(0, nq, 97, device=dev), torch.tensor([nq - 1], device=dev)])
    q[zero] = 0.0
    s_r, i_r = ops.retrieve_topk(q, c, k, mode="f16r")
    s_p, i_p = ops.retrieve_topk(q, c, k, mode="f16r", prepared=ops.retrieve_prepare(c, mode="f16r"))
    assert torch.equal(s_r, s_p) and torch.equal(i_r, i_p)
    del s_p, i_p
    s_x, i_x = ops.retrieve_topk(q, c, k, mode="bf16x3")
    ar = torch.arange(k, dtype=torch.int32, device=dev).expand(zero.numel(), k)
    for s, i in ((s_r, i_r), (s_x, i_x)):
        assert torch.equal(i[zero], ar) and bool((s[zero] == 0).all())
    # the aligned queries: the k lowest-index copies of the hot row
    hot_sorted = hot.sort().values[:k].to(torch.int32)
    assert torch.equal(i_r[aligned], hot_sorted.expand(aligned.numel(), k))
    kth, nxt, worst, err_own, err_rank, scale = _vs_fp64_in_blocks(q, c, k, s_r, i_r)
    tol = 1e-5 * scale
    assert err_own <= tol                              # every reported score is its index's score
    assert err_rank <= tol                             # the reported scores are the k best, best first
    assert float((kth - worst).max()) <= tol           # nothing from below the cut but near-ties of it
    si_r, si_x = i_r.sort(dim=1).values, i_x.sort(dim=1).values
    assert bool((si_r[:, 1:] != si_r[:, :-1]).all())   # k distinct indices per row
    clear = (kth - nxt) > tol
    assert bool((si_r == si_x).all(dim=1)[clear].all()), "f16r and bf16x3 index sets differ on a row without a near-tie"
    del q, c, s_r, i_r, s_x, i_x, si_r, si_x
    torch.cuda.empty_cache()


# ---- b. the plan sweep: hundreds of chunks per call through the measuring hooks --------------------------------------
# (nq, N, D, k, index_base, index_step, zero query rows)
SWEEP = [(1, 70_001, 512, 500, 0, 1, ()),
         (1, 30_000, 130, 1, 1 << 20, 7, (0,)),
         (64, 30_000, 130, 1024, 3, 2, (0, 31)),
         (64, 70_001, 96, 500, 11, 5, (63,)),
         (257, 70_001, 96, 1, 0, 1, (5, 256)),
         (257, 30_000, 512, 1024, 0, 1, (100,))]


@functools.lru_cache(maxsize=None)
def _sweep_case(n):
    """grid-valued queries (some zero) and candidates with duplicated rows -- scattered pairs, and a run of copies that
    straddles the end of the first chunk -- and the oracle's answer"""
    nq, N_, D, k, _, _, zeros = SWEEP[n]
    rng = np.random.default_rng(4000 + n)
    q, c = _grid(rng, (nq, D)), _grid(rng, (N_, D))
    q[list(zeros)] = 0.0
    c[rng.integers(0, N_, 300)] = c[rng.integers(0, N_, 300)]
    f = _first(N_, k)
    c[f - 20:f + 20] = c[rng.integers(0, N_)]
    es, ei = o_topk.batched_top_k(q, c, k, F64)
    return q, c, es, ei


@pytest.mark.parametrize("lazy", [None, "0"], ids=["lazy", "compact_every_chunk"])
@pytest.mark.parametrize("cap", [128, 1000])
@pytest.mark.parametrize("case", range(len(SWEEP)), ids=["nq%d_N%d_D%d_k%d" % s[:4] for s in SWEEP])
def test_retrieve_plan_sweep_exact_arithmetic(dev, monkeypatch, case, cap, lazy):
    """Regime: ESR_RETRIEVE_LIST_LOG2=20 and ESR_RETRIEVE_CHUNK_CAP = 128 or 1000 (not a multiple of the 128-row tile:
    chunks start inside a tile) -> later chunks of 128 or 1000 rows: 107 - 485 chunks per call at the cap of 128, 14 - 63
    at 1000;
    ppitch = mark + chunk = 1664 - 4072, below f16r's first chunk of 8192 / 16 384 (the f16r list is `first` long).
    Lazy compaction on, or ESR_RETRIEVE_LAZY=0 (a select after every chunk).  Every mode, plain and prepared, bit for bit
    against the oracle; ties everywhere (grid values, zero queries, duplicated rows), index_base / index_step."""
    from esrecsys_amd import ops
    monkeypatch.setenv("ESR_RETRIEVE_LIST_LOG2", "20")
    monkeypatch.setenv("ESR_RETRIEVE_CHUNK_CAP", str(cap))
    if lazy is None:
        monkeypatch.delenv("ESR_RETRIEVE_LAZY", raising=False)
    else:
        monkeypatch.setenv("ESR_RETRIEVE_LAZY", lazy)
    monkeypatch.setattr(ops, "_ws_size_cache", {})     # the hooks change the workspace size of the same arguments
    q, c, es, ei = _sweep_case(case)
    _, _, _, k, base, step, _ = SWEEP[case]
    _all_modes_bit_exact(dev, q, c, k, es, ei, base, step)


# ---- c. chunk boundaries of the default plan --------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first-1", "first", "first+1", "first+127", "first+128", "first+chunk+1", "k"])
@pytest.mark.parametrize("k", [7, 512, 1024])
def test_retrieve_chunk_boundaries_exact_arithmetic(dev, k, where):
    """Regime: default plan at 37 queries (chunk = the 65 536 cap, ppitch > first): N one short of the first chunk
    (first = 8192 for k <= 512, 16 384 for k = 1024), equal to it, one row and a tile (less one) past it, a second chunk
    of exactly one tile, a third chunk of one row, and N = k (every candidate is in the answer).  Every mode, plain and
    prepared, bit for bit against the oracle.  At N = first + 1 the last candidate's reported index is 2^31 - 1."""
    nq, D = 37, 96
    first = 16_384 if k > 512 else 8192
    N_ = {"first-1": first - 1, "first": first, "first+1": first + 1, "first+127": first + 127,
          "first+128": first + 128, "first+chunk+1": first + 65_536 + 1, "k": k}[where]
    rng = np.random.default_rng(N_ * 3 + k)
    q, c = _grid(rng, (nq, D)), _grid(rng, (N_, D))
    q[3] = 0.0
    c[N_ - 1] = c[0]                                   # the last candidate (in the last chunk) ties the first
    c[rng.integers(0, N_, 50)] = c[rng.integers(0, N_, 50)]
    es, ei = o_topk.batched_top_k(q, c, k, F64)
    base, step = (2 ** 31 - 1 - (N_ - 1) * 3, 3) if where == "first+1" else (0, 1)
    _all_modes_bit_exact(dev, q, c, k, es, ei, base, step)


# ---- d. a prepared corpus belongs to the candidates as they were ---------------------------------------------------------
def test_prepared_corpus_refuses_candidates_changed_in_place(dev):
    """retrieve_prepare records the candidates' version counter and keeps the tensor: an in-place update (a training
    step) after the prepare is refused -- the planes and the largest norm f16r's band is built on would be stale -- while
    the untouched matrix, or a view of it, is accepted; a fresh prepare of the updated matrix is accepted again."""
    from esrecsys_amd import ops
    from esrecsys_amd.pinterest.make_recommendations import find_top_k_batch
    g = torch.Generator(device=dev).manual_seed(3)
    q = torch.randn((16, 64), generator=g, device=dev)
    c = torch.randn((10_000, 64), generator=g, device=dev)
    prep = ops.retrieve_prepare(c, mode="f16r")
    s0, i0 = ops.retrieve_topk(q, c, 20, mode="f16r")
    s1, i1 = ops.retrieve_topk(q, c, 20, mode="f16r", prepared=prep)
    assert torch.equal(s0, s1) and torch.equal(i0, i1)
    s2, i2 = ops.retrieve_topk(q, c.view(10_000, 64), 20, mode="f16r", prepared=prep)
    assert torch.equal(s0, s2) and torch.equal(i0, i2)
    c.mul_(2)
    with pytest.raises(ValueError):
        ops.retrieve_topk(q, c, 20, mode="f16r", prepared=prep)
    with pytest.raises(ValueError):
        find_top_k_batch(q, c, 20, prepared=prep)
    s3, i3 = ops.retrieve_topk(q, c, 20, mode="f16r", prepared=ops.retrieve_prepare(c, mode="f16r"))
    s4, i4 = ops.retrieve_topk(q, c, 20, mode="f16r")
    assert torch.equal(s3, s4) and torch.equal(i3, i4) and torch.equal(i4, i0)

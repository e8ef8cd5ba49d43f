"""Implicit-feedback ALS on one MI355X: the user and the item half-sweep of ``factorization.ImplicitALS`` at ranks 32 and 64
on the Dice benchmark's corpus (benchmarks/dice_bench.py: 1 M Zipf documents of about 20 ids; user = document) and on the
large synthetic corpus of benchmarks/als_bench.py (140 000 users, 27 000 items, about 20 M pairs).  Per half-sweep: the wall
time, every kernel's time by HIP events (the two Gram kernels and the row-class kernels), the Gram kernel against the time
its table takes at the HBM peak, the explicit ``als_solve_rows`` on the same CSR in the same session, and a plain-torch
restatement (``index_add_`` of weighted outer products + ``Y^T Y`` + batched Cholesky) on a slice of the rows, with both
compared against the same restatement in fp64.  Reported context, not a target: ``split_holdout`` on the Dice corpus ->
``recommend_documents`` (k = 500) -> ``ranking_metrics``, beside item-kNN on the same split.  Prints JSON lines.

    python benchmarks/ials_bench.py [--reps 3] [--inner 3] [--skip_large] [--skip_torch] [--skip_quality]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from als_bench import HBM_BYTES_PER_S, ULP32, _kernel_times, _windows, device_corpus, row_errors  # noqa: E402


def torch_half_sweep(Y, offsets, cols, weights, reg, weighted, dtype, slab):
    """The implicit half-sweep in plain torch: Y^T Y once, the weighted Gram matrices and right-hand sides by index_add_ of
    outer products over slabs of `slab` entries, then a batched Cholesky solve.  (Atomic adds: no fixed order.)"""
    dev = Y.device
    n_rows, rank = offsets.numel() - 1, Y.shape[1]
    counts = offsets[1:] - offsets[:-1]
    row = torch.repeat_interleave(torch.arange(n_rows, device=dev), counts)
    Yd = Y.to(dtype)
    G = (Yd.t() @ Yd)[None].repeat(n_rows, 1, 1)
    b = torch.zeros((n_rows, rank), dtype=dtype, device=dev)
    base = int(offsets[0])
    for s in range(0, row.numel(), slab):
        e = min(s + slab, row.numel())
        y = Yd[cols[base + s:base + e].to(torch.int64)]
        w = weights[base + s:base + e].to(dtype)
        G.index_add_(0, row[s:e], (y * w[:, None])[:, :, None] * y[:, None, :])
        b.index_add_(0, row[s:e], y * (1 + w)[:, None])
        del y
    lam = torch.full((n_rows,), float(np.float32(reg)), dtype=dtype, device=dev)
    if weighted:
        lam = lam * counts.to(dtype)
    G.diagonal(dim1=1, dim2=2).add_(lam[:, None])
    L = torch.linalg.cholesky(G)
    del G
    x = torch.cholesky_solve(b[:, :, None], L)[:, :, 0]
    return torch.where((counts > 0)[:, None], x, torch.zeros_like(x))          # a row without entries: zeros


def bench_config(name, model, args, dev, lib, with_torch):
    from esrecsys_amd import ops
    rank, reg, wreg = model.rank, model.reg, model.weighted_reg
    nnz, nu, ni = model.nnz, int(model.users.numel()), int(model.items.numel())
    rec = {"bench": "ials", "corpus": name, "rank": rank, "pairs": nnz, "users": nu, "items": ni, "alpha": model.alpha,
           "reg": reg, "longest_user_row": int(np.diff(model._user_offsets).max()),
           "longest_item_row": int(np.diff(model._item_offsets).max()), "chunk": ops.als_geometry()[0],
           "gram_segment": ops.als_gram_geometry()}
    model.sweep()                                  # warm-up: code objects, the LDS limit, the allocator
    model.sweep()
    failed = torch.zeros(1, dtype=torch.int32, device=dev)
    sides = (("user", model.item_factors, model._user_offsets, model._row_ipos, model._weights, model.user_factors,
              model.solve_users),
             ("item", model.user_factors, model._item_offsets, model._col_upos, model._weights_by_item, model.item_factors,
              model.solve_items))
    for side, Y, off, cols, w, out, solve in sides:
        n_rows = off.size - 1
        t_imp = min(_windows(solve, args.reps, args.inner))
        # the explicit solve on the same CSR (the weights as targets), into a scratch table, in the same session
        scratch = torch.zeros_like(out)
        explicit = lambda: ops.als_solve_rows(Y, off, cols, w, 0, n_rows, reg, wreg, scratch, failed)   # noqa: E731
        explicit()
        t_exp = min(_windows(explicit, args.reps, args.inner))
        gram = lambda: ops.als_gram(Y)                                                               # noqa: E731
        t_gram = min(_windows(gram, args.reps, args.inner))
        lib.esr_kernel_timing(1)
        solve()
        torch.cuda.synchronize()
        kernels = _kernel_times(lib)
        lib.esr_kernel_timing(0)
        seg_ms = kernels.get("als_gram_segments", {}).get("ms", float("nan"))
        table_bytes = int(Y.shape[0]) * rank * 4
        rec[side] = {"rows": n_rows, "half_sweep_ms": round(t_imp * 1e3, 4), "explicit_half_sweep_ms": round(t_exp * 1e3, 4),
                     "implicit_over_explicit": round(t_imp / t_exp, 3), "gram_call_ms": round(t_gram * 1e3, 4),
                     "kernels_one_half_sweep": kernels, "gram_table_bytes": table_bytes,
                     "gram_segments_kernel_fraction_of_hbm_peak": round(table_bytes / (seg_ms * 1e-3) / HBM_BYTES_PER_S, 5),
                     "pairs_per_s": round(nnz / t_imp)}
        del scratch
        if with_torch:
            rows = min(n_rows, args.torch_rows)
            off_d = torch.from_numpy(off[:rows + 1]).to(dev)
            G = ops.als_gram(Y)
            got = torch.zeros((rows, rank), dtype=torch.float32, device=dev)
            call = lambda: ops.als_solve_rows_implicit(Y, G, off, cols, w, 0, rows, reg, wreg, got, failed)   # noqa: E731
            call()
            t_k = min(_windows(call, args.reps, args.inner))
            slab = max(1 << 12, (1 << 28) // (rank * rank))      # about 1 GiB of f32 outer products per slab
            torch_half_sweep(Y[:64], off_d[:9].clamp(max=8), cols[:8].clamp(max=63), w[:8], reg, wreg, torch.float32, slab)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x32 = torch_half_sweep(Y, off_d, cols, w, reg, wreg, torch.float32, slab)
            torch.cuda.synchronize()
            t32 = time.perf_counter() - t0
            x64 = torch_half_sweep(Y, off_d, cols, w, reg, wreg, torch.float64, slab // 2)
            ek, et = row_errors(got, x64), row_errors(x32, x64)
            rec[side].update({"torch_rows": rows, "torch_restatement_ms": round(t32 * 1e3, 3),
                              "kernel_same_rows_ms": round(t_k * 1e3, 4), "torch_over_kernel": round(t32 / t_k, 2),
                              "kernel_error_vs_fp64_max": float(ek.max()), "torch_f32_error_vs_fp64_max": float(et.max()),
                              "equal_within_tolerance": bool(float(ek.max()) <= 4 * float(et.max()) + 8 * ULP32)})
            del x32, x64, got, ek, et, G
            torch.cuda.empty_cache()
    return rec


def quality(ctx, c_off, truth, t_off, kept, args, dev):
    """The hold-out pipeline on the Dice corpus: ImplicitALS on the contexts, recommend_documents for the first `queries`
    kept documents, ranking_metrics -- and item-kNN (Dice neighbours) on the same split."""
    from esrecsys_amd import evaluate
    from esrecsys_amd import factorization as fz
    from esrecsys_amd.wikipedia import neighbours as nbm
    from esrecsys_amd.wikipedia.make_dice import DiceBuilder
    nq = min(args.queries, int(kept.numel()))
    q_ctx, q_off = ctx[:int(c_off[nq])], c_off[:nq + 1]
    q_truth, q_toff = truth[:int(t_off[nq])], t_off[:nq + 1]
    out = {"bench": "ials", "stage": "hold_out_context", "documents": int(kept.numel()), "queries": nq, "k": 500}
    t0 = time.perf_counter()
    model = fz.ImplicitALS.from_documents(ctx, c_off, rank=32, device=dev)
    history = model.fit(sweeps=args.quality_sweeps)
    ids, _, lens = model.recommend_documents(q_ctx, q_off, k=500)
    torch.cuda.synchronize()
    m = evaluate.ranking_metrics(ids, lens, q_truth, q_toff, ks=(10, 100, 500)).mean()
    out["ials"] = {"rank": 32, "sweeps": args.quality_sweeps, "objective_first": history[0], "objective_last": history[-1],
                   "objective_non_increasing": bool(all(b <= a * (1 + 1e-6) for a, b in zip(history, history[1:]))),
                   "recall": [float(x) for x in m["recall"]], "ndcg": [float(x) for x in m["ndcg"]],
                   "seconds": round(time.perf_counter() - t0, 2)}
    del model
    t0 = time.perf_counter()
    b = DiceBuilder(capacity=1 << 20, device=dev).add(ctx, c_off)
    index, other, count = b.finalize()
    d_ids, df = b.doc_frequency()
    table = nbm.neighbours(index, other, count, d_ids, df, 20, "both", "dice")
    ids, _, lens = nbm.recommend(table, q_ctx, q_off, 500)
    torch.cuda.synchronize()
    m = evaluate.ranking_metrics(ids, lens, q_truth, q_toff, ks=(10, 100, 500)).mean()
    out["item_knn"] = {"neighbours": 20, "recall": [float(x) for x in m["recall"]], "ndcg": [float(x) for x in m["ndcg"]],
                       "seconds": round(time.perf_counter() - t0, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--torch_rows", type=int, default=131072)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--quality_sweeps", type=int, default=3)
    ap.add_argument("--skip_large", action="store_true")
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    args = ap.parse_args()
    from dice_bench import _corpus
    from esrecsys_amd import _lib
    from esrecsys_amd import factorization as fz
    from esrecsys_amd.evaluate import split_holdout
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC
    assert torch.cuda.is_available(), "ials_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    print(json.dumps({"bench": "ials", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "calls_per_window": args.inner, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S}), flush=True)
    indices, off = _corpus(np.random.default_rng(0), args.docs, args.vocab, 20, 1.2, 2000, MAX_DOC)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)
    for rank in (32, 64):
        model = fz.ImplicitALS.from_documents(d_indices, d_off, rank=rank, device=dev)
        print(json.dumps(bench_config("dice_bench", model, args, dev, lib, not args.skip_torch)), flush=True)
        del model
        torch.cuda.empty_cache()
    if not args.skip_large:
        user, item, _, _ = device_corpus(140000, 27000, 156, 1.1, 20.0, dev, seed=2)
        for rank in (32, 64):
            model = fz.ImplicitALS(user, item, rank=rank, device=dev)
            print(json.dumps(bench_config("synthetic_20M", model, args, dev, lib, not args.skip_torch)), flush=True)
            del model
            torch.cuda.empty_cache()
    if not args.skip_quality:
        ctx, c_off, truth, t_off, kept = split_holdout(d_indices, d_off)
        print(json.dumps(quality(ctx, c_off, truth, t_off, kept, args, dev)), flush=True)


if __name__ == "__main__":
    main()

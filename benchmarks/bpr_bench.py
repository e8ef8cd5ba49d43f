"""BPR on one MI355X: the training step of ``factorization.BPR`` at rank 64 and B = 65 536 on the Dice benchmark's corpus
(benchmarks/dice_bench.py: 1 M Zipf documents of about 20 ids) split by ``split_holdout``; the model is trained on the
contexts (user = kept document).  Per step: the time of the sampler, the forward / backward kernel, the sort and the update
by HIP events, the wall time of ``train_steps``, triples per second, and the forward / backward kernel against the time its
own bytes (6 rows of D floats and 16 bytes of ids per triple) take at the HBM peak.  The same step restated in plain torch
(gather, logsigmoid, ``index_add_`` per distinct row, Adagrad on the touched rows) runs in the same session on the same
triples.  Reported context, not a target: hold-out recall and nDCG at 10 / 100 / 500 of ``recommend`` for the first
`queries` kept documents, beside iALS and item-kNN on the same split (benchmarks/ials_bench.py's ``quality``).  Prints JSON
lines.

    python benchmarks/bpr_bench.py [--reps 3] [--steps 64] [--train_steps 3000] [--skip_torch] [--skip_quality]
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

from als_bench import HBM_BYTES_PER_S, _windows  # noqa: E402
from ials_bench import quality as ials_and_knn_quality  # noqa: E402


def phase_times(model, K):
    """ms per step of the four phases of K steps, by HIP events on the stream (the steps really train)."""
    from esrecsys_amd import ops
    ev = lambda: torch.cuda.Event(enable_timing=True)                        # noqa: E731
    marks = [[ev() for _ in range(5)] for _ in range(K)]
    s0, s1 = ev(), ev()
    s0.record()
    u, i, j, valid, _ = model.sample(K)
    s1.record()
    nu, ni = int(model.users.numel()), int(model.items.numel())
    for k in range(K):
        m = marks[k]
        m[0].record()
        _, _, grads = ops.bpr_fwd_bwd(model.user_factors, model.item_factors, u[k], i[k], j[k], valid[k], model.reg,
                                      failed=model._failed)
        m[1].record()
        sorted_ids, perm = ops.segment_sort_multi([u[k], i[k], j[k]], [0, nu, nu], nu + ni)
        m[2].record()
        ops.sparse_adagrad_multi([model.user_factors, model.item_factors], [model.user_accum, model.item_accum],
                                 [0, nu, nu + ni], sorted_ids, perm, grads, model.lr)
        m[3].record()
    torch.cuda.synchronize()
    model.step += K
    med = lambda a, b: float(np.median([m[a].elapsed_time(m[b]) for m in marks]))   # noqa: E731
    return {"sample_ms": s0.elapsed_time(s1) / K, "fwd_bwd_ms": med(0, 1), "sort_ms": med(1, 2), "update_ms": med(2, 3)}


def torch_step(U, Y, Ua, Ya, u, i, j, valid, reg, lr, eps=1e-7):
    """One step in plain torch on given triples (int64 ids): returns the summed loss (device scalar)."""
    x, yi, yj = U[u], Y[i], Y[j]
    df = yi - yj
    d = (x * df).sum(1)
    keep = valid.to(torch.float32)
    loss = -(torch.nn.functional.logsigmoid(d) * keep).sum()
    g = (torch.sigmoid(-d) * keep)[:, None]
    k2 = keep[:, None]
    gu, gi, gj = -g * df + reg * k2 * x, -g * x + reg * k2 * yi, g * x + reg * k2 * yj
    for table, acc, ids, rows in ((U, Ua, u, gu), (Y, Ya, torch.cat([i, j]), torch.cat([gi, gj]))):
        touched, inv = torch.unique(ids, return_inverse=True)
        G = torch.zeros((touched.numel(), table.shape[1]), dtype=torch.float32, device=table.device).index_add_(0, inv, rows)
        a = acc[touched] + G * G
        acc[touched] = a
        table[touched] -= lr * G * torch.where(a > 0, torch.rsqrt(a + eps), torch.zeros_like(a))
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64, help="steps per timed window")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--train_steps", type=int, default=3000)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--quality_sweeps", type=int, default=3)
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    args = ap.parse_args()
    from dice_bench import _corpus
    from esrecsys_amd import evaluate
    from esrecsys_amd import factorization as fz
    from esrecsys_amd import ops
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC
    assert torch.cuda.is_available(), "bpr_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    print(json.dumps({"bench": "bpr", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "steps_per_window": args.steps, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
                      "geometry": ops.bpr_geometry()}), flush=True)
    indices, off = _corpus(np.random.default_rng(0), args.docs, args.vocab, 20, 1.2, 2000, MAX_DOC)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)
    ctx, c_off, truth, t_off, kept = evaluate.split_holdout(d_indices, d_off)
    t0 = time.perf_counter()
    model = fz.BPR.from_documents(ctx, c_off, rank=args.rank, batch=args.batch, device=dev)
    torch.cuda.synchronize()
    D, B = model.rank, model.batch
    rec = {"bench": "bpr", "stage": "step", "corpus": "dice_bench contexts", "rank": D, "batch": B, "pairs": model.nnz,
           "users": int(model.users.numel()), "items": int(model.items.numel()), "optimizer": model.optimizer, "lr": model.lr,
           "reg": model.reg, "build_seconds": round(time.perf_counter() - t0, 2)}
    model.train_steps(8)                                   # warm-up: code objects, the allocator
    wall = min(_windows(lambda: model.train_steps(args.steps), args.reps, 1)) / args.steps
    phases = phase_times(model, args.steps)
    bytes_fb = (6 * D * 4 + 16) * B
    rec.update({"train_steps_ms_per_step": round(wall * 1e3, 4), "triples_per_s": round(B / wall),
                **{k: round(v, 4) for k, v in phases.items()},
                "phases_sum_ms": round(sum(phases.values()), 4), "fwd_bwd_bytes_per_triple": 6 * D * 4 + 16,
                "fwd_bwd_fraction_of_hbm_peak": round(bytes_fb / (phases["fwd_bwd_ms"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "dropped_per_step_mean": float(model.sample(8)[4].to(torch.float64).mean())})
    print(json.dumps(rec), flush=True)
    if not args.skip_torch:
        K = min(args.steps, 16)
        u, i, j, valid, _ = (t.to(torch.int64) for t in model.sample(K))
        U, Y = model.user_factors.clone(), model.item_factors.clone()
        Ua, Ya = model.user_accum.clone(), model.item_accum.clone()
        torch_step(U, Y, Ua, Ya, u[0], i[0], j[0], valid[0], model.reg, model.lr)           # warm-up
        state = {"k": 0}

        def one():
            k = state["k"] % K
            state["k"] += 1
            torch_step(U, Y, Ua, Ya, u[k], i[k], j[k], valid[k], model.reg, model.lr)
        t_torch = min(_windows(one, args.reps, K))
        # the kernel path on the same triples and a copy of the tables, sampler left out on both sides
        m2 = {"U": model.user_factors.clone(), "Y": model.item_factors.clone(), "Ua": model.user_accum.clone(),
              "Ya": model.item_accum.clone()}
        u32, i32, j32, v32 = (t.to(torch.int32).contiguous() for t in (u, i, j, valid))
        nu, ni = int(model.users.numel()), int(model.items.numel())
        failed = torch.zeros(1, dtype=torch.int32, device=dev)

        def ours():
            k = state["k"] % K
            state["k"] += 1
            loss_t, _, grads = ops.bpr_fwd_bwd(m2["U"], m2["Y"], u32[k], i32[k], j32[k], v32[k], model.reg, failed=failed)
            s, p = ops.segment_sort_multi([u32[k], i32[k], j32[k]], [0, nu, nu], nu + ni)
            ops.sparse_adagrad_multi([m2["U"], m2["Y"]], [m2["Ua"], m2["Ya"]], [0, nu, nu + ni], s, p, grads, model.lr)
            loss_t.to(torch.float64).sum()
        ours()
        t_ours = min(_windows(ours, args.reps, K))
        print(json.dumps({"bench": "bpr", "stage": "torch_restatement", "rank": D, "batch": B, "steps_per_window": K,
                          "torch_ms_per_step": round(t_torch * 1e3, 4), "kernels_ms_per_step": round(t_ours * 1e3, 4),
                          "torch_over_kernels": round(t_torch / t_ours, 2)}), flush=True)
        del U, Y, Ua, Ya, m2
        torch.cuda.empty_cache()
    if not args.skip_quality:
        nq = min(args.queries, int(kept.numel()))
        q_truth, q_toff = truth[:int(t_off[nq])], t_off[:nq + 1]
        del model                                          # the timed model has taken steps: the quality leg trains a fresh one
        t0 = time.perf_counter()
        model = fz.BPR.from_documents(ctx, c_off, rank=args.rank, batch=args.batch, device=dev)
        auc0 = model.auc()
        losses = model.fit(args.train_steps)
        ids, _, lens = model.recommend(torch.arange(nq, device=dev), k=500)
        torch.cuda.synchronize()
        m = evaluate.ranking_metrics(ids, lens, q_truth, q_toff, ks=(10, 100, 500)).mean()
        out = ials_and_knn_quality(ctx, c_off, truth, t_off, kept, args, dev)
        out.update({"bench": "bpr", "stage": "hold_out_context"})
        out["bpr"] = {"rank": D, "batch": B, "steps": model.step, "epochs": round(model.step * B / model.nnz, 1),
                      "loss_first": float(np.mean(losses[:10])), "loss_last": float(np.mean(losses[-10:])),
                      "auc_before": auc0, "auc_after": model.auc(),
                      "recall": [float(x) for x in m["recall"]], "ndcg": [float(x) for x in m["ndcg"]],
                      "seconds": round(time.perf_counter() - t0, 2)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

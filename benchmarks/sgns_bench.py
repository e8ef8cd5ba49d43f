"""SGNS on one MI355X: the training step of ``factorization.SGNS`` at rank 64, B = 65 536, window 5 and 5 noise items on the
planted-successor corpus of ``fpmc_bench`` (1 M documents of about 20 ids over 200 000 Zipf ids), trained on the sequences
without their last id (``evaluate.split_last``).  Per step: the time of the sampler, the forward / backward kernel, the sort
and the update by HIP events, the wall time of ``train_steps``, slots per second, and the forward / backward kernel against
the time its own bytes -- ``(2 + K) * 2 * 4 D`` of rows read and written plus ``4 (3 + K) + 4`` of ids and loss per slot --
take at the HBM peak.  The same step restated in plain torch runs in the same session on the same slots.  Hold-out next-item
recall and nDCG at 10 of ``recommend_sequences`` under ``split_last`` beside FPMC (window 1) trained as long, both at
`quality_rank`.  Prints JSON lines.

    python benchmarks/sgns_bench.py [--reps 3] [--steps 32] [--train_steps 1500] [--skip_torch] [--skip_quality]
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
from fpmc_bench import planted_corpus  # noqa: E402


def phase_times(model, K):
    """ms per step of the four phases of K steps, by HIP events on the stream (the steps really train)."""
    from esrecsys_amd import ops
    ev = lambda: torch.cuda.Event(enable_timing=True)                        # noqa: E731
    marks = [[ev() for _ in range(4)] for _ in range(K)]
    s0, s1 = ev(), ev()
    s0.record()
    c, _, o, valid, neg, _ = model.sample(K)
    context = torch.cat([o[:, None, :], neg.permute(0, 2, 1)], 1).contiguous()
    s1.record()
    ni = int(model.items.numel())
    tables, accums = [model.in_factors, model.out_factors], [model.in_accum, model.out_accum]
    for k in range(K):
        m = marks[k]
        m[0].record()
        _, _, grads = ops.sgns_fwd_bwd(*tables, c[k], o[k], neg[k], valid[k], model.reg, failed=model._failed)
        m[1].record()
        sorted_ids, perm = ops.segment_sort_multi([c[k], context[k].reshape(-1)], [0, ni], 2 * ni)
        m[2].record()
        ops.sparse_adagrad_multi(tables, accums, [0, ni, 2 * ni], sorted_ids, perm, grads, model.lr)
        m[3].record()
    torch.cuda.synchronize()
    model.step += K
    med = lambda a, b: float(np.median([m[a].elapsed_time(m[b]) for m in marks]))   # noqa: E731
    return {"sample_ms": s0.elapsed_time(s1) / K, "fwd_bwd_ms": med(0, 1), "sort_ms": med(1, 2), "update_ms": med(2, 3)}


def torch_step(tables, accums, c, o, neg, valid, reg, lr, eps=1e-7):
    """One SGNS step in plain torch on given slots (int64): returns the summed loss (device scalar)."""
    V, W = tables
    v, wo, wn = V[c], W[o], W[neg]                                            # [B, D], [B, D], [B, K, D]
    keep = valid.to(torch.float32)
    m = (neg != o[:, None]).to(torch.float32) * keep[:, None]
    so, sk = (v * wo).sum(1), (v[:, None, :] * wn).sum(2)
    loss = (torch.nn.functional.softplus(-so) * keep).sum() + (torch.nn.functional.softplus(sk) * m).sum()
    ao, ak = (torch.sigmoid(so) - 1.0) * keep, torch.sigmoid(sk) * m
    k2 = keep[:, None]
    gc = ao[:, None] * wo + (ak[:, :, None] * wn).sum(1) + reg * k2 * v
    go = ao[:, None] * v + reg * k2 * wo
    gn = ak[:, :, None] * v[:, None, :] + reg * m[:, :, None] * wn
    for table, acc, ids, rows in ((V, accums[0], c, gc),
                                  (W, accums[1], torch.cat([o, neg.reshape(-1)]), torch.cat([go, gn.reshape(-1, v.shape[1])]))):
        touched, inv = torch.unique(ids, return_inverse=True)
        G = torch.zeros((touched.numel(), table.shape[1]), dtype=torch.float32, device=table.device).index_add_(0, inv, rows)
        a = acc[touched] + G * G
        acc[touched] = a
        table[touched] -= lr * G * torch.where(a > 0, torch.rsqrt(a + eps), torch.zeros_like(a))
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32, help="steps per timed window")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--follow", type=float, default=0.5)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negatives", type=int, default=5)
    ap.add_argument("--quality_rank", type=int, default=32)
    ap.add_argument("--train_steps", type=int, default=1500)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    args = ap.parse_args()
    from esrecsys_amd import evaluate
    from esrecsys_amd import factorization as fz
    from esrecsys_amd import ops
    assert torch.cuda.is_available(), "sgns_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    print(json.dumps({"bench": "sgns", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "steps_per_window": args.steps, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "follow": args.follow,
                      "geometry": ops.sgns_geometry()}), flush=True)
    indices, off = planted_corpus(np.random.default_rng(0), args.docs, args.vocab, 20, args.follow)
    train, train_off, truth, t_off, kept = evaluate.split_last(torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev))
    D, B, K = args.rank, args.batch, args.negatives
    t0 = time.perf_counter()
    model = fz.SGNS.from_documents(train, train_off, window=args.window, negatives=K, rank=D, batch=B, device=dev)
    torch.cuda.synchronize()
    rec = {"bench": "sgns", "stage": "step", "window": args.window, "negatives": K, "rank": D, "batch": B,
           "events": model.n_events, "items": int(model.items.numel()), "optimizer": model.optimizer,
           "build_seconds": round(time.perf_counter() - t0, 2)}
    model.train_steps(8)                                   # warm-up: code objects, the allocator
    wall = min(_windows(lambda: model.train_steps(args.steps), args.reps, 1)) / args.steps
    phases = phase_times(model, args.steps)
    dropped = float(model.sample(args.steps)[5].to(torch.float64).mean()) / B
    per_slot = (2 + K) * 2 * 4 * D + 4 * (3 + K) + 4
    engine = phases["sort_ms"] + phases["update_ms"]
    rec.update({"train_steps_ms_per_step": round(wall * 1e3, 4), "slots_per_s": round(B / wall),
                **{k: round(v, 4) for k, v in phases.items()}, "phases_sum_ms": round(sum(phases.values()), 4),
                "engine_share_of_phases": round(engine / sum(phases.values()), 3), "dropped_share": round(dropped, 4),
                "engine_rows_per_step": (2 + K) * B, "fwd_bwd_bytes_per_slot": per_slot,
                "fwd_bwd_fraction_of_hbm_peak": round(per_slot * B / (phases["fwd_bwd_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)})
    print(json.dumps(rec), flush=True)
    if not args.skip_torch:
        steps = min(args.steps, 8)
        c, _, o, valid, neg, _ = (t.to(torch.int64) for t in model.sample(steps))
        tables = [model.in_factors.clone(), model.out_factors.clone()]
        accums = [torch.full_like(t, 0.1) for t in tables]
        state = {"k": 0}

        def one():
            k = state["k"] % steps
            state["k"] += 1
            torch_step(tables, accums, c[k], o[k], neg[k], valid[k], model.reg, model.lr)
        one()
        t_torch = min(_windows(one, args.reps, steps))
        kernels = sum(phases.values()) - phases["sample_ms"]
        print(json.dumps({"bench": "sgns", "stage": "torch_restatement", "rank": D, "batch": B, "steps_per_window": steps,
                          "torch_ms_per_step": round(t_torch * 1e3, 4), "kernels_ms_per_step": round(kernels, 4),
                          "torch_over_kernels": round(t_torch * 1e3 / kernels, 2)}), flush=True)
        del tables, accums
    del model
    torch.cuda.empty_cache()
    if not args.skip_quality:
        nq = min(args.queries, int(kept.numel()))
        q_truth, q_toff = truth[:int(t_off[nq])], t_off[:nq + 1]
        q_ids, q_off = train[:int(train_off[nq])], train_off[:nq + 1]
        out = {"bench": "sgns", "stage": "hold_out_next_item", "protocol": "split_last", "queries": nq,
               "rank": args.quality_rank, "batch": B, "steps": args.train_steps, "follow": args.follow}
        kw = dict(rank=args.quality_rank, batch=B, device=dev)
        for name, make in (("sgns", lambda: fz.SGNS.from_documents(train, train_off, window=args.window, negatives=K, **kw)),
                           ("sgns_window1", lambda: fz.SGNS.from_documents(train, train_off, window=1, negatives=K, **kw)),
                           ("fpmc_window1", lambda: fz.FPMC.from_documents(train, train_off, window=1, **kw))):
            t0 = time.perf_counter()
            model = make()
            losses = model.fit(args.train_steps)
            ids, _, lens = model.recommend_sequences(q_ids, q_off, k=10, exclude_seen=False)
            torch.cuda.synchronize()
            m = evaluate.ranking_metrics(ids, lens, q_truth, q_toff, ks=(10,)).mean()
            out[name] = {"loss_first": float(np.mean(losses[:10])), "loss_last": float(np.mean(losses[-10:])),
                         "recall_at_10": float(m["recall"][0]), "ndcg_at_10": float(m["ndcg"][0]),
                         "seconds": round(time.perf_counter() - t0, 2)}
            del model
            torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

"""FPMC on one MI355X: the training step of ``factorization.FPMC`` at rank 64 and B = 65 536, window 1 and 3, on a corpus of
the Dice benchmark's shape (1 M documents of about 20 ids over 200 000 Zipf ids) whose documents are SEQUENCES with a
planted first-order structure: with probability `follow` an id's successor is a fixed function of the id, otherwise a Zipf
draw.  The model is trained on the sequences without their last id (``evaluate.split_last``).  Per step: the time of the
sampler, the forward / backward kernel, the sort and the update by HIP events, the wall time of ``train_steps``, slots per
second, and the forward / backward kernel against the time its own bytes -- ``(5 + c) * 2 * 4 D`` of rows read and written
plus ``4 (6 + 2 c)`` of ids per slot, c the mean context length -- take at the HBM peak.  BPR's step on the same corpus
stands beside it, and the same FPMC step restated in plain torch runs in the same session on the same slots.  Hold-out
next-item recall and nDCG at 10 under ``split_last`` for FPMC against BPR trained as long, both at `quality_rank` (serving
re-scores rows of 2 rank by the ALS predict kernel: rank <= 64).  Prints JSON lines.

    python benchmarks/fpmc_bench.py [--reps 3] [--steps 32] [--train_steps 1500] [--skip_torch] [--skip_quality]
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
from bpr_bench import phase_times as bpr_phase_times  # noqa: E402


def planted_corpus(rng, docs, vocab, mean_len, follow, exponent=1.2):
    """(indices int64, offsets int64[docs + 1]): documents of 3 + Poisson(mean_len - 3) ids; the first id and every jump
    are Zipf(exponent) draws over a shuffled vocabulary, and with probability `follow` an id is followed by its successor
    ``succ[id]``, a fixed random permutation."""
    lengths = 3 + rng.poisson(mean_len - 3, docs)
    width = int(lengths.max())
    p = 1.0 / np.arange(1, vocab + 1) ** exponent
    cdf = np.cumsum(p / p.sum())
    names = rng.permutation(vocab)
    draw = lambda n: names[np.minimum(np.searchsorted(cdf, rng.random(n)), vocab - 1)]      # noqa: E731
    succ = rng.permutation(vocab)
    seqs = np.empty((docs, width), np.int64)
    seqs[:, 0] = draw(docs)
    for t in range(1, width):
        seqs[:, t] = np.where(rng.random(docs) < follow, succ[seqs[:, t - 1]], draw(docs))
    inside = np.arange(width)[None, :] < lengths[:, None]
    return seqs[inside], np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def phase_times(model, K):
    """ms per step of the four phases of K steps, by HIP events on the stream (the steps really train)."""
    from esrecsys_amd import ops
    ev = lambda: torch.cuda.Event(enable_timing=True)                        # noqa: E731
    marks = [[ev() for _ in range(4)] for _ in range(K)]
    s0, s1 = ev(), ev()
    s0.record()
    u, e, c, i, j, valid, _ = model.sample(K)
    oo = torch.zeros((K, model.batch + 1), dtype=torch.int64, device=model.device)
    oo[:, 1:] = torch.cumsum(c, 1)
    ij = torch.cat([i, j], dim=1)
    s1.record()
    totals = oo[:, -1].cpu().numpy()
    nu, ni = int(model.users.numel()), int(model.items.numel())
    tables = model._tables()
    accums = [model.user_accum, model.item_accum, model.next_accum, model.prev_accum]
    for k in range(K):
        m = marks[k]
        m[0].record()
        _, _, grads, ctx_ids = ops.fpmc_fwd_bwd(*tables, model._seq_ipos, u[k], e[k], c[k], i[k], j[k], valid[k], model.reg,
                                                ctx_offsets=oo[k], M=int(totals[k]), failed=model._failed)
        m[1].record()
        sorted_ids, perm = ops.segment_sort_multi([u[k], ij[k], ij[k], ctx_ids], [0, nu, nu + ni, nu + 2 * ni], nu + 3 * ni)
        m[2].record()
        ops.sparse_adagrad_multi(tables, accums, [0, nu, nu + ni, nu + 2 * ni, nu + 3 * ni], sorted_ids, perm, grads, model.lr)
        m[3].record()
    torch.cuda.synchronize()
    model.step += K
    model._served = None
    med = lambda a, b: float(np.median([m[a].elapsed_time(m[b]) for m in marks]))   # noqa: E731
    return {"sample_and_scan_ms": s0.elapsed_time(s1) / K, "fwd_bwd_ms": med(0, 1), "sort_ms": med(1, 2),
            "update_ms": med(2, 3)}, float(totals.mean()) / model.batch


def torch_step(tables, accums, seq, u, e, c, i, j, valid, window, reg, lr, eps=1e-7):
    """One FPMC step in plain torch on given slots (int64): returns the summed loss (device scalar)."""
    U, A, Bn, P = tables
    n = torch.arange(window, device=u.device)[None, :]
    mask = n < c[:, None]
    L = seq[torch.where(mask, (e - c)[:, None] + n, torch.zeros_like(n))]
    w = (1.0 / c.clamp(min=1).to(torch.float32))[:, None]
    pl = P[L] * mask[:, :, None]
    m = pl.sum(1) * w
    x, ai, aj, bi, bj = U[u], A[i], A[j], Bn[i], Bn[j]
    da, db = ai - aj, bi - bj
    d = (x * da).sum(1) + (m * db).sum(1)
    keep = valid.to(torch.float32)
    loss = -(torch.nn.functional.logsigmoid(d) * keep).sum()
    g = (torch.sigmoid(-d) * keep)[:, None]
    k2 = keep[:, None]
    gm = -g * db
    gp = ((w * gm)[:, None, :] + reg * k2[:, None, :] * pl)[mask]
    ij = torch.cat([i, j])
    for table, acc, ids, rows in ((U, accums[0], u, -g * da + reg * k2 * x),
                                  (A, accums[1], ij, torch.cat([-g * x + reg * k2 * ai, g * x + reg * k2 * aj])),
                                  (Bn, accums[2], ij, torch.cat([-g * m + reg * k2 * bi, g * m + reg * k2 * bj])),
                                  (P, accums[3], L[mask], gp)):
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
    ap.add_argument("--quality_rank", type=int, default=32)
    ap.add_argument("--train_steps", type=int, default=1500)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    args = ap.parse_args()
    from esrecsys_amd import evaluate
    from esrecsys_amd import factorization as fz
    from esrecsys_amd import ops
    assert torch.cuda.is_available(), "fpmc_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    print(json.dumps({"bench": "fpmc", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "steps_per_window": args.steps, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "follow": args.follow,
                      "geometry": ops.fpmc_geometry()}), flush=True)
    indices, off = planted_corpus(np.random.default_rng(0), args.docs, args.vocab, 20, args.follow)
    train, train_off, truth, t_off, kept = evaluate.split_last(torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev))
    D, B = args.rank, args.batch
    for window in (1, 3):
        t0 = time.perf_counter()
        model = fz.FPMC.from_documents(train, train_off, window=window, rank=D, batch=B, device=dev)
        torch.cuda.synchronize()
        rec = {"bench": "fpmc", "stage": "step", "window": window, "rank": D, "batch": B, "events": model.n_events,
               "pairs": model.nnz, "users": int(model.users.numel()), "items": int(model.items.numel()),
               "optimizer": model.optimizer, "build_seconds": round(time.perf_counter() - t0, 2)}
        model.train_steps(8)                               # warm-up: code objects, the allocator
        wall = min(_windows(lambda: model.train_steps(args.steps), args.reps, 1)) / args.steps
        phases, c_mean = phase_times(model, args.steps)
        per_slot = (5 + c_mean) * 2 * 4 * D + 4 * (6 + 2 * c_mean)
        engine = phases["sort_ms"] + phases["update_ms"]
        rec.update({"train_steps_ms_per_step": round(wall * 1e3, 4), "slots_per_s": round(B / wall),
                    **{k: round(v, 4) for k, v in phases.items()}, "phases_sum_ms": round(sum(phases.values()), 4),
                    "engine_share_of_phases": round(engine / sum(phases.values()), 3), "context_mean": round(c_mean, 3),
                    "engine_rows_per_step": round((5 + c_mean) * B), "fwd_bwd_bytes_per_slot": round(per_slot, 1),
                    "fwd_bwd_fraction_of_hbm_peak": round(per_slot * B / (phases["fwd_bwd_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)})
        print(json.dumps(rec), flush=True)
        if not args.skip_torch and window == 3:
            K = min(args.steps, 8)
            u, e, c, i, j, valid, _ = (t.to(torch.int64) for t in model.sample(K))
            tables, accums = [t.clone() for t in model._tables()], [torch.full_like(t, 0.1) for t in model._tables()]
            seq = model._seq_ipos.to(torch.int64)
            state = {"k": 0}

            def one():
                k = state["k"] % K
                state["k"] += 1
                torch_step(tables, accums, seq, u[k], e[k], c[k], i[k], j[k], valid[k], window, model.reg, model.lr)
            one()
            t_torch = min(_windows(one, args.reps, K))
            print(json.dumps({"bench": "fpmc", "stage": "torch_restatement", "window": window, "rank": D, "batch": B,
                              "steps_per_window": K, "torch_ms_per_step": round(t_torch * 1e3, 4),
                              "kernels_ms_per_step": round((sum(phases.values()) - phases["sample_and_scan_ms"]), 4),
                              "torch_over_kernels": round(t_torch * 1e3 / (sum(phases.values()) - phases["sample_and_scan_ms"]),
                                                          2)}), flush=True)
            del tables, accums
        del model
        torch.cuda.empty_cache()
    bpr = fz.BPR.from_documents(train, train_off, rank=D, batch=B, device=dev)
    bpr.train_steps(8)
    wall = min(_windows(lambda: bpr.train_steps(args.steps), args.reps, 1)) / args.steps
    phases = bpr_phase_times(bpr, args.steps)
    print(json.dumps({"bench": "fpmc", "stage": "bpr_step_beside_it", "rank": D, "batch": B,
                      "train_steps_ms_per_step": round(wall * 1e3, 4), **{k: round(v, 4) for k, v in phases.items()},
                      "phases_sum_ms": round(sum(phases.values()), 4)}), flush=True)
    del bpr
    torch.cuda.empty_cache()
    if not args.skip_quality:
        nq = min(args.queries, int(kept.numel()))
        q_truth, q_toff = truth[:int(t_off[nq])], t_off[:nq + 1]
        users = torch.arange(nq, device=dev)
        out = {"bench": "fpmc", "stage": "hold_out_next_item", "protocol": "split_last", "queries": nq,
               "rank": args.quality_rank, "batch": B, "steps": args.train_steps, "follow": args.follow}
        kw = dict(rank=args.quality_rank, batch=B, device=dev)
        for name, make in (("fpmc_window1", lambda: fz.FPMC.from_documents(train, train_off, window=1, **kw)),
                           ("fpmc_window3", lambda: fz.FPMC.from_documents(train, train_off, window=3, **kw)),
                           ("bpr", lambda: fz.BPR.from_documents(train, train_off, **kw))):
            t0 = time.perf_counter()
            model = make()
            losses = model.fit(args.train_steps)
            ids, _, lens = model.recommend(users, k=10, exclude_seen=False)
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

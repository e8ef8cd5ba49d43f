"""WARP on one MI355X: the training step of ``factorization.WARP`` at rank 64, B = 65 536 and max_trials = 32 on the corpus
and split of benchmarks/bpr_bench.py (the Dice benchmark's 1 M Zipf documents, ``split_holdout``, user = kept document).
Per step: the time of the fused ``warp_step`` kernel, the sort and the update by HIP events, the wall time of
``train_steps``, and the kernel against the time its own bytes take at the HBM peak -- per slot two rows read, one row
per scored candidate (the measured mean trials), three gradient rows written and 28 bytes of ids; the probes of the row
search are left out, so the fraction is a lower bound on the traffic.  The step restated in plain torch (all T candidates
gathered as [B, T, D], ``bmm``, first violator by ``argmax``, weight, ``index_add_`` per distinct row, Adagrad on the
touched rows) runs in the same session.  Then a fresh model is trained for `train_steps` steps: ``mean_trials`` at steps 0,
1000 and the last, and hold-out recall and nDCG at 10 / 100 / 500 beside ``BPR`` trained as long on the same split.
Reported, not targets.  Prints JSON lines.

    python benchmarks/warp_bench.py [--reps 3] [--steps 64] [--train_steps 3000] [--skip_torch] [--skip_quality]
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


def phase_times(model, K):
    """ms per step of the three phases of K steps, by HIP events on the stream (the steps really train), and the mean
    trials per slot of those steps."""
    ev = lambda: torch.cuda.Event(enable_timing=True)                        # noqa: E731
    marks = [[ev() for _ in range(4)] for _ in range(K)]
    total = torch.zeros((), dtype=torch.float64, device=model.device)
    for k in range(K):
        m = marks[k]
        m[0].record()
        u, i, j, valid, trials, _, _, grads = model._warp_step(model.step + k, True)
        m[1].record()
        model._update(u, i, j, grads)                                        # (the sort and the update; timed apart below)
        m[2].record()
        total += trials.sum()
    torch.cuda.synchronize()
    model.step += K
    med = lambda a, b: float(np.median([m[a].elapsed_time(m[b]) for m in marks]))   # noqa: E731
    return {"warp_step_ms": med(0, 1), "sort_and_update_ms": med(1, 2)}, float(total) / (K * model.batch)


def sort_update_split(model, K):
    """the sort and the update apart, on the triples of one step (the tables move, as in training)"""
    from esrecsys_amd import ops
    ev = lambda: torch.cuda.Event(enable_timing=True)                        # noqa: E731
    nu, ni = int(model.users.numel()), int(model.items.numel())
    u, i, j, _, _, _, _, grads = model._warp_step(model.step, True)
    marks = [[ev() for _ in range(3)] for _ in range(K)]
    for m in marks:
        m[0].record()
        sorted_ids, perm = ops.segment_sort_multi([u, i, j], [0, nu, nu], nu + ni)
        m[1].record()
        ops.sparse_adagrad_multi([model.user_factors, model.item_factors], [model.user_accum, model.item_accum],
                                 [0, nu, nu + ni], sorted_ids, perm, grads, model.lr)
        m[2].record()
    torch.cuda.synchronize()
    med = lambda a, b: float(np.median([m[a].elapsed_time(m[b]) for m in marks]))   # noqa: E731
    return {"sort_ms": med(0, 1), "update_ms": med(1, 2)}


def torch_step(U, Y, Ua, Ya, key, row_len, weight, nnz, T, margin, reg, lr, B, gen, eps=1e-7):
    """One WARP step in plain torch: pairs and candidates from torch's generator, every candidate scored."""
    ni = Y.shape[0]
    p = torch.randint(0, nnz, (B,), device=U.device, generator=gen)
    u, i = key[p] >> 32, key[p] & 0xFFFFFFFF
    cand = torch.randint(0, ni, (B, T), device=U.device, generator=gen)
    probe = (u[:, None] << 32) | cand
    at = torch.searchsorted(key, probe.reshape(-1)).clamp_(max=nnz - 1).reshape(B, T)
    unseen = key[at] != probe
    x, yi = U[u], Y[i]
    s_i = (x * yi).sum(1)
    s_j = torch.bmm(Y[cand], x[:, :, None])[:, :, 0]                         # [B, T, D] x [B, D, 1]
    viol = unseen & ((s_i[:, None] - s_j) < margin)
    valid = viol.any(1)
    first = viol.to(torch.int8).argmax(1)
    N = (unseen.cumsum(1).gather(1, first[:, None])[:, 0]).clamp_(min=1)
    j = cand.gather(1, first[:, None])[:, 0]
    r = ((ni - row_len[u]) // N).clamp_(min=1)
    w = (weight[r] * valid)[:, None]
    k2 = valid.to(torch.float32)[:, None]
    yj = Y[j]
    gu, gi, gj = reg * k2 * x - w * (yi - yj), reg * k2 * yi - w * x, reg * k2 * yj + w * x
    for table, acc, ids, rows in ((U, Ua, u, gu), (Y, Ya, torch.cat([i, j]), torch.cat([gi, gj]))):
        touched, inv = torch.unique(ids, return_inverse=True)
        G = torch.zeros((touched.numel(), table.shape[1]), dtype=torch.float32, device=table.device).index_add_(0, inv, rows)
        a = acc[touched] + G * G
        acc[touched] = a
        table[touched] -= lr * G * torch.where(a > 0, torch.rsqrt(a + eps), torch.zeros_like(a))


def hold_out(model, nq, q_truth, q_toff, dev):
    from esrecsys_amd import evaluate
    ids, _, lens = model.recommend(torch.arange(nq, device=dev), k=500)
    torch.cuda.synchronize()
    m = evaluate.ranking_metrics(ids, lens, q_truth, q_toff, ks=(10, 100, 500)).mean()
    return {"recall": [float(x) for x in m["recall"]], "ndcg": [float(x) for x in m["ndcg"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64, help="steps per timed window")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--max_trials", type=int, default=32)
    ap.add_argument("--train_steps", type=int, default=3000)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    args = ap.parse_args()
    from dice_bench import _corpus
    from esrecsys_amd import evaluate
    from esrecsys_amd import factorization as fz
    from esrecsys_amd import ops
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC
    assert torch.cuda.is_available(), "warp_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    print(json.dumps({"bench": "warp", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "steps_per_window": args.steps, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
                      "geometry": ops.warp_geometry()}), flush=True)
    indices, off = _corpus(np.random.default_rng(0), args.docs, args.vocab, 20, 1.2, 2000, MAX_DOC)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)
    ctx, c_off, truth, t_off, kept = evaluate.split_holdout(d_indices, d_off)
    kw = dict(rank=args.rank, batch=args.batch, device=dev)
    t0 = time.perf_counter()
    model = fz.WARP.from_documents(ctx, c_off, max_trials=args.max_trials, **kw)
    torch.cuda.synchronize()
    D, B, T = model.rank, model.batch, model.max_trials
    rec = {"bench": "warp", "stage": "step", "corpus": "dice_bench contexts", "rank": D, "batch": B, "max_trials": T,
           "margin": model.margin, "rank_weight": "harmonic", "pairs": model.nnz, "users": int(model.users.numel()),
           "items": int(model.items.numel()), "optimizer": model.optimizer, "lr": model.lr, "reg": model.reg,
           "build_seconds": round(time.perf_counter() - t0, 2)}
    model.train_steps(8)                                   # warm-up: code objects, the allocator
    wall = min(_windows(lambda: model.train_steps(args.steps), args.reps, 1)) / args.steps
    phases, trials = phase_times(model, args.steps)
    phases.update(sort_update_split(model, args.steps))
    bytes_slot = (2 + trials + 3) * D * 4 + 28
    rec.update({"train_steps_ms_per_step": round(wall * 1e3, 4), "slots_per_s": round(B / wall),
                **{k: round(v, 4) for k, v in phases.items()}, "steps_taken_when_timed": model.step,
                "mean_trials_when_timed": round(trials, 3), "warp_step_bytes_per_slot": round(bytes_slot, 1),
                "warp_step_fraction_of_hbm_peak": round(bytes_slot * B / (phases["warp_step_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)})
    print(json.dumps(rec), flush=True)
    if not args.skip_torch:
        U, Y = model.user_factors.clone(), model.item_factors.clone()
        Ua, Ya = model.user_accum.clone(), model.item_accum.clone()
        row_len = torch.from_numpy(np.diff(model._user_offsets)).to(dev)
        gen = torch.Generator(device=dev).manual_seed(0)
        one = lambda: torch_step(U, Y, Ua, Ya, model._key, row_len, model.rank_weight, model.nnz, T, model.margin, model.reg,   # noqa: E731
                                 model.lr, B, gen)
        one()
        t_torch = min(_windows(one, args.reps, 8))
        print(json.dumps({"bench": "warp", "stage": "torch_restatement", "rank": D, "batch": B, "max_trials": T,
                          "torch_ms_per_step": round(t_torch * 1e3, 4), "kernels_ms_per_step": round(wall * 1e3, 4),
                          "torch_over_kernels": round(t_torch / wall, 2)}), flush=True)
        del U, Y, Ua, Ya
        torch.cuda.empty_cache()
    if not args.skip_quality:
        nq = min(args.queries, int(kept.numel()))
        q_truth, q_toff = truth[:int(t_off[nq])], t_off[:nq + 1]
        del model                                          # the timed model has taken steps: the quality leg trains fresh ones
        out = {"bench": "warp", "stage": "hold_out_context", "queries": nq, "train_steps": args.train_steps}
        for name, make in (("warp", lambda: fz.WARP.from_documents(ctx, c_off, max_trials=args.max_trials, **kw)),
                           ("bpr", lambda: fz.BPR.from_documents(ctx, c_off, **kw))):
            t0 = time.perf_counter()
            model = make()
            auc0 = model.auc()
            losses = model.fit(args.train_steps)
            torch.cuda.synchronize()
            seconds = time.perf_counter() - t0
            out[name] = {"rank": D, "batch": B, "steps": model.step, "loss_first": float(np.nanmean(losses[:10])),
                         "loss_last": float(np.nanmean(losses[-10:])), "auc_before": auc0, "auc_after": model.auc(),
                         "fit_seconds": round(seconds, 2), **hold_out(model, nq, q_truth, q_toff, dev)}
            if name == "warp":
                mt = model.mean_trials
                out[name]["mean_trials"] = {"step_0": mt[0], "step_1000": mt[min(1000, len(mt) - 1)], "step_last": mt[-1]}
            del model
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

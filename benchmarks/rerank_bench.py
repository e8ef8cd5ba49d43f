"""Diversity re-ranking on one MI355X: a BPR model on the Dice benchmark's corpus split by ``split_holdout`` (as
benchmarks/bpr_bench.py), ``recommend(k=500)`` for 8192 kept documents, then ``diversify(n=100, lam=0.7)`` -- the time of
the whole call and of its kernel (HIP events), the kernel's HBM and LDS bytes against their peaks, beside the same rule
restated in plain torch in the same session: gather [nq, k, D], one ``bmm`` for all similarities, n rounds of masked
``argmax`` / ``maximum`` (in slabs of queries: the [nq, k, k] similarities of all 8192 do not fit).  Reported context, not a
target: intra-list similarity, coverage and hold-out recall / nDCG at 10 / 100 before and after.  Prints JSON lines.

    python benchmarks/rerank_bench.py [--reps 3] [--train_steps 1000] [--queries 8192] [--k 500] [--n 100] [--lam 0.7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from als_bench import HBM_BYTES_PER_S, _windows  # noqa: E402

LDS_BYTES_PER_S = 256 * 128 * 2.4e9      # 256 CUs x 128 bytes per clock (ds_read_b128) x 2.4 GHz


def torch_mmr(pos, rel, lengths, rows, lam, n, slab=512):
    """The rule of rerank.mmr in plain torch: picked list positions int64[nq, n], -1 behind a list's end."""
    nq, k = pos.shape
    lam32 = torch.tensor(lam, dtype=torch.float32, device=rows.device)
    oml = 1.0 - lam32
    out = torch.full((nq, n), -1, dtype=torch.int64, device=rows.device)
    col = torch.arange(k, device=rows.device)[None, :]
    for a in range(0, nq, slab):
        b = min(nq, a + slab)
        R = rows[pos[a:b].clamp(min=0).to(torch.int64)]
        S = torch.bmm(R, R.transpose(1, 2))
        live = col < lengths[a:b, None]
        r, m, ar = rel[a:b], None, torch.arange(b - a, device=rows.device)
        for t in range(n):
            v = lam32 * r if m is None else lam32 * r - oml * m
            v = torch.where(live, v, torch.full_like(v, -float("inf")))
            s = torch.argmax(v, dim=1)
            out[a:b, t] = torch.where(live[ar, s], s, torch.full_like(s, -1))
            live[ar, s] = False
            sim = S[ar, s]
            m = sim if m is None else torch.maximum(m, sim)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--train_steps", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--k", type=int, default=500)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--skip_torch", action="store_true")
    args = ap.parse_args()
    from dice_bench import _corpus
    from esrecsys_amd import evaluate, ops, rerank
    from esrecsys_amd import factorization as fz
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC
    assert torch.cuda.is_available(), "rerank_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    geom = ops.rerank_geometry(args.rank, args.k)
    print(json.dumps({"bench": "rerank", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
                      "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "lds_peak_bytes_per_s": LDS_BYTES_PER_S, "geometry": geom}),
          flush=True)
    indices, off = _corpus(np.random.default_rng(0), args.docs, args.vocab, 20, 1.2, 2000, MAX_DOC)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)
    ctx, c_off, truth, t_off, kept = evaluate.split_holdout(d_indices, d_off)
    model = fz.BPR.from_documents(ctx, c_off, rank=args.rank, batch=args.batch, device=dev)
    model.fit(args.train_steps)
    nq, k, n, D = min(args.queries, int(kept.numel())), args.k, args.n, args.rank
    q_truth, q_toff = truth[:int(t_off[nq])], t_off[:nq + 1]
    ids, scores, lens = model.recommend(torch.arange(nq, device=dev), k=k)
    torch.cuda.synchronize()

    def call():
        return model.diversify(ids, scores, lens, lam=args.lam, n=n)
    d_ids, d_scores, d_lens = call()                                           # warm-up: the code object, the LDS limit
    t_call = min(_windows(call, args.reps, 1))
    rows = rerank.unit_rows(model.item_factors)
    pos = model._positions(ids.reshape(-1), model.items).reshape(nq, k)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernel_ms = []
    for _ in range(args.reps):
        e0.record()
        picked = ops.rerank_mmr(rows, pos, scores, lens, args.lam, n, failed=word)[0]
        e1.record()
        torch.cuda.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    t_kernel = min(kernel_ms) * 1e-3
    mean_len = float(lens.to(torch.float64).mean())
    hbm = nq * (mean_len * (D * 4 + 8) + 16 * n + 4)                             # rows once, cand and rel, the outputs
    lds = nq * n * mean_len * (D * 4 + 12)                                       # per round every candidate's row and state
    rec = {"bench": "rerank", "stage": "mmr", "queries": nq, "k": k, "n": n, "lam": args.lam, "rank": D,
           "items": int(model.items.numel()), "mean_list_length": round(mean_len, 1), "staged": geom["staged"],
           "diversify_ms": round(t_call * 1e3, 3), "kernel_ms": round(t_kernel * 1e3, 3),
           "kernel_us_per_query": round(t_kernel * 1e6 / nq, 3), "kernel_hbm_bytes": int(hbm), "kernel_lds_bytes": int(lds),
           "kernel_fraction_of_hbm_peak": round(hbm / t_kernel / HBM_BYTES_PER_S, 4),
           "kernel_fraction_of_lds_peak": round(lds / t_kernel / LDS_BYTES_PER_S, 4)}
    if not args.skip_torch:
        lens64 = lens.to(torch.int64)
        t_pos = torch_mmr(pos[:1024], scores[:1024], lens64[:1024], rows, args.lam, n)        # warm-up
        t_torch = min(_windows(lambda: torch_mmr(pos, scores, lens64, rows, args.lam, n), args.reps, 1))
        t_pos = torch_mmr(pos, scores, lens64, rows, args.lam, n)
        same = (t_pos == picked.to(torch.int64)).all(1)
        rec.update({"torch_ms": round(t_torch * 1e3, 3), "torch_over_kernel": round(t_torch / t_kernel, 2),
                    "torch_over_diversify": round(t_torch / t_call, 2), "lists_equal_to_torch": int(same.sum()),
                    "winner": "kernel" if t_kernel < t_torch else "torch"})
    print(json.dumps(rec), flush=True)
    out = {"bench": "rerank", "stage": "quality", "ks": [10, 100]}
    d_pos = model._positions(d_ids.reshape(-1), model.items).reshape(nq, n)
    for name, (i_, l_, p_) in (("recommend", (ids, lens, pos)), ("diversify", (d_ids, d_lens, d_pos))):
        m = evaluate.ranking_metrics(i_, l_, q_truth, q_toff, ks=(10, 100)).mean()
        ils = rerank.intra_list_similarity(p_, l_, rows, ks=(10, 100)).mean()
        out[name] = {"recall": [float(x) for x in m["recall"]], "ndcg": [float(x) for x in m["ndcg"]],
                     "ils": [float(x) for x in ils["ils"]], "coverage": rerank.coverage(i_, l_, (10, 100)).tolist()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

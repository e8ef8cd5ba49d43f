"""Offline evaluation on one MI355X, on the corpus of benchmarks/dice_bench.py (1 M Zipf documents): split_holdout (first
5 ids in, the rest held out) -> DiceBuilder on the contexts -> neighbours(k = 20) -> recommend(k = 500) for 8192 held-out
queries -> ranking_metrics at (10, 100, 500).  Then ranking_metrics alone at nq = 8192 and nq = 1 000 000 (width 500, truth
lengths as the corpus gives), beside the torch restatement of the same hit counts in the same session -- pad the truth
lists, sort, searchsorted: spotify.train_spotify._recall's form, which counts every list position that holds a truth id,
i.e. count_repeats -- whose counts must equal the kernel's.  One JSON line per stage; the quality figures are what item-kNN
reaches on this synthetic corpus, not targets.

    python benchmarks/eval_bench.py [--docs 1000000] [--vocab 200000] [--queries 8192] [--big 1000000] [--reps 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM = 8e12   # bytes/s, the MI355X's HBM3E peak
_NO_ID = 1 << 40


def _timed(fn, reps):
    out, times = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def torch_hits(rec_ids, truth, off, chunk=65536):
    """Per query: how many list positions hold one of its truth ids.  The truth lists padded to the longest of a chunk of
    queries, sorted, probed with searchsorted (plain torch; cut into chunks because the pad is [queries, longest] int64)."""
    nq = rec_ids.shape[0]
    out = torch.empty(nq, dtype=torch.int64, device=rec_ids.device)
    lens = off[1:] - off[:-1]
    for a in range(0, nq, chunk):
        b = min(nq, a + chunk)
        n = lens[a:b]
        L = max(int(n.max()), 1)
        col = torch.arange(L, device=rec_ids.device)
        live = col[None, :] < n[:, None]
        at = torch.where(live, off[a:b, None] + col[None, :], torch.zeros((), dtype=torch.int64, device=rec_ids.device))
        pad = torch.where(live, truth[at].long(), torch.full((), _NO_ID, dtype=torch.int64, device=rec_ids.device))
        pad = pad.sort(dim=1).values
        ids = rec_ids[a:b].long()
        pos = torch.searchsorted(pad, ids).clamp_(max=L - 1)
        out[a:b] = (pad.gather(1, pos) == ids).sum(dim=1)
    return out


def _metrics_stage(lib, name, rec_ids, rec_lengths, truth, off, ks, reps):
    from dice_bench import _kernel_times
    from esrecsys_amd.evaluate import ranking_metrics
    nq, width = rec_ids.shape
    run = lambda: ranking_metrics(rec_ids, rec_lengths, truth, off, ks=ks)                   # noqa: E731
    run()
    m, t = _timed(run, reps)
    lib.esr_kernel_timing(1)
    run()
    torch.cuda.synchronize()
    kernels = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    # the reference's count -- every position that holds a truth id -- from the kernel and from torch
    counted = lambda: ranking_metrics(rec_ids, None, truth, off, ks=(width,), count_repeats=True,   # noqa: E731
                                      truth_size="listed")
    counted()
    mc, t_c = _timed(counted, reps)
    ref = lambda: torch_hits(rec_ids, truth, off)                                            # noqa: E731
    ref()
    r_hits, t_ref = _timed(ref, reps)
    same = bool(torch.equal(r_hits, mc.hits[:, 0].long()))
    nk = len(ks)
    out_bytes = nq * (24 * nk + 8)
    algo = 4 * nq * width + 4 * int(truth.numel()) + 8 * (nq + 1) + out_bytes + (4 * nq if rec_lengths is not None else 0)
    k_ms = kernels.get("eval_ranking", {}).get("ms")
    best = min(t)
    mean = m.mean()
    rec = {"bench": "eval", "stage": name, "queries": nq, "width": width, "ks": list(ks), "truth_ids": int(truth.numel()),
           "truth_longest": int((off[1:] - off[:-1]).max()), "reps": reps, "ms": round(best * 1e3, 3),
           "ms_all": [round(x * 1e3, 3) for x in t], "queries_per_s": round(nq / best), "kernels_ms": kernels,
           "algorithmic_bytes": algo, "kernel_bytes_per_s": round(algo / (k_ms * 1e-3)) if k_ms else None,
           "kernel_fraction_of_8TBps": round(algo / (k_ms * 1e-3) / HBM, 4) if k_ms else None,
           "call_fraction_of_8TBps": round(algo / best / HBM, 4),
           "count_form": {"ms": round(min(t_c) * 1e3, 3), "ms_all": [round(x * 1e3, 3) for x in t_c]},
           "torch_restatement": {"ms": round(min(t_ref) * 1e3, 3), "ms_all": [round(x * 1e3, 3) for x in t_ref],
                                 "equal_to_kernel_hits": same, "kernel_speedup": round(min(t_ref) / min(t_c), 2)},
           "n_valid": mean["n_valid"],
           "quality": {key: [round(float(v), 6) for v in mean[key]] for key in ("precision", "recall", "rr", "ap", "ndcg")}}
    print(json.dumps(rec), flush=True)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--mean", type=int, default=20)
    ap.add_argument("--tail", type=int, default=2000)
    ap.add_argument("--zipf", type=float, default=1.2)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--big", type=int, default=1_000_000)
    ap.add_argument("--rec_k", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from dice_bench import _corpus
    from esrecsys_amd import _lib
    from esrecsys_amd.evaluate import split_holdout
    from esrecsys_amd.wikipedia import neighbours as nbm
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC, DiceBuilder
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    ks = (10, 100, 500)
    indices, off = _corpus(np.random.default_rng(0), args.docs, args.vocab, args.mean, args.zipf, args.tail, MAX_DOC)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)

    split = lambda: split_holdout(d_indices, d_off)                                          # noqa: E731
    split()
    (ctx, c_off, truth, t_off, kept), t_split = _timed(split, args.reps)
    print(json.dumps({"bench": "eval", "stage": "split_holdout", "docs": args.docs, "ids": int(off[-1]),
                      "kept": int(kept.numel()), "context_ids": int(ctx.numel()), "truth_ids": int(truth.numel()),
                      "ms": round(min(t_split) * 1e3, 3), "ms_all": [round(x * 1e3, 3) for x in t_split]}), flush=True)

    DiceBuilder(capacity=1 << 10, device=dev).add(indices[:off[3]], off[:4]).finalize()     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = DiceBuilder(capacity=1 << 20, device=dev).add(ctx, c_off)
    index, other, count = b.finalize()
    ids, df = b.doc_frequency()
    table = nbm.neighbours(index, other, count, ids, df, args.k, "both", "dice")
    torch.cuda.synchronize()
    print(json.dumps({"bench": "eval", "stage": "dice_builder_and_neighbours", "nnz": int(index.numel()),
                      "rows": int(ids.numel()), "k": args.k, "ms": round((time.perf_counter() - t0) * 1e3, 3)}), flush=True)
    del index, other, count

    def lists(nq):
        """the lists of the first nq held-out queries (the kept documents taken round and round)"""
        n_kept = int(kept.numel())
        rec = torch.empty((nq, args.rec_k), dtype=torch.int32, device=dev)
        rec_len = torch.empty(nq, dtype=torch.int32, device=dev)
        tr, tr_off = [], [torch.zeros(1, dtype=torch.int64, device=dev)]
        done = 0
        while done < nq:
            n = min(nq - done, n_kept, 131072)
            a = done % n_kept
            n = min(n, n_kept - a)
            h = ctx[c_off[a]:c_off[a + n]]
            r_ids, _, r_len = nbm.recommend(table, h, c_off[a:a + n + 1] - c_off[a], args.rec_k)
            rec[done:done + n], rec_len[done:done + n] = r_ids, r_len
            tr.append(truth[t_off[a]:t_off[a + n]])
            tr_off.append(t_off[a + 1:a + n + 1] - t_off[a] + tr_off[-1][-1])
            done += n
        return rec, rec_len, torch.cat(tr), torch.cat(tr_off)

    for name, nq in (("ranking_metrics_%d" % args.queries, args.queries), ("ranking_metrics_%d" % args.big, args.big)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec, rec_len, tr, tr_off = lists(nq)
        torch.cuda.synchronize()
        print(json.dumps({"bench": "eval", "stage": "recommend", "queries": nq, "k": args.rec_k,
                          "mean_length": round(float(rec_len.float().mean()), 2),
                          "ms": round((time.perf_counter() - t0) * 1e3, 3)}), flush=True)
        _metrics_stage(lib, name, rec, rec_len, tr, tr_off, ks, args.reps)
        del rec, rec_len, tr, tr_off


if __name__ == "__main__":
    main()

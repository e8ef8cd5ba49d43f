"""Neighbour table and item-kNN recommender on one MI355X, on the corpus of benchmarks/dice_bench.py (1 M Zipf documents):
DiceBuilder -> neighbours(k = 20, "both") -> recommend for 8192 queries of 5 ids, k = 500.  One JSON line per stage:
rows/s, entries/s and the achieved bytes/s against the stage's algorithmic bytes at 8 TB/s, with the per-kernel times.
Beside the neighbour stage, in the same session on the same GPU, a plain-torch restatement: the symmetric entry list
sorted by a composite key (torch.sort of (inverted score bits, partner), then a stable sort by row), then per-row slices
-- its table must equal the kernel's.

    python benchmarks/neighbours_bench.py [--docs 1000000] [--vocab 200000] [--k 20] [--queries 8192] [--reps 5]
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


def _timed(fn, reps):
    """(result, seconds of each repeat): the host clock around work that ends in a device synchronise."""
    out, times = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def _kernels(lib, fn):
    from dice_bench import _kernel_times
    lib.esr_kernel_timing(1)
    fn()
    torch.cuda.synchronize()
    out = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    return out


def torch_neighbours(index, other, count, ids, df, k):
    """The restatement: plain torch on the same GPU.  (neighbours, scores, lengths) of the symmetric matrix."""
    ids64 = ids.to(torch.int64)
    pi, po = torch.searchsorted(ids64, index.to(torch.int64)), torch.searchsorted(ids64, other.to(torch.int64))
    s = count / (df[po] + df[pi])
    row, partner, score = torch.cat([pi, po]), torch.cat([other, index]).to(torch.int64), torch.cat([s, s])
    bits = score.view(torch.int32).to(torch.int64)            # scores are positive: their bits order them
    key = ((0x7FFFFFFF - bits) << 31) | partner               # score descending, partner id ascending
    key, order = torch.sort(key)
    row, order2 = torch.sort(row[order], stable=True)
    key = key[order2]
    u = ids.numel()
    start = torch.searchsorted(row, torch.arange(u + 1, device=row.device))
    length = torch.clamp(start[1:] - start[:-1], max=k)
    col = torch.arange(k, device=row.device)
    live = col[None, :] < length[:, None]
    at = torch.where(live, start[:-1, None] + col[None, :], torch.zeros((), dtype=torch.int64, device=row.device))
    kept = key[at] if key.numel() else torch.zeros((u, k), dtype=torch.int64, device=row.device)
    nb = torch.where(live, kept & 0x7FFFFFFF, torch.full((), -1, dtype=torch.int64, device=row.device)).to(torch.int32)
    sc = torch.where(live, (0x7FFFFFFF - (kept >> 31)).to(torch.int32).view(torch.float32),
                     torch.zeros((), device=row.device))
    return nb, sc, length.to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--mean", type=int, default=20)
    ap.add_argument("--tail", type=int, default=2000)
    ap.add_argument("--zipf", type=float, default=1.2)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--history", type=int, default=5)
    ap.add_argument("--rec_k", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from dice_bench import _corpus
    from esrecsys_amd import _lib
    from esrecsys_amd.wikipedia import neighbours as nbm
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC, DiceBuilder
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    indices, off = _corpus(rng, args.docs, args.vocab, args.mean, args.zipf, args.tail, MAX_DOC)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)

    # stage 1: the matrix
    DiceBuilder(capacity=1 << 10, device=dev).add(indices[:off[3]], off[:4]).finalize()   # warm-up
    built = {}

    def build():
        b = DiceBuilder(capacity=built.get("capacity", 1 << 20), device=dev)
        b.add(d_indices, d_off)
        out = b.finalize() + b.doc_frequency()
        built["capacity"] = b.capacity
        return out

    build()                                                                                 # sizes the table
    (index, other, count, ids, df), t_build = _timed(build, 2)
    nnz, u = index.numel(), ids.numel()
    print(json.dumps({"bench": "neighbours", "stage": "dice_builder", "docs": args.docs, "ids": int(off[-1]),
                      "vocab": args.vocab, "nnz": nnz, "rows": u, "ms": round(min(t_build) * 1e3, 3),
                      "ms_all": [round(t * 1e3, 3) for t in t_build], "docs_per_s": round(args.docs / min(t_build))}))

    # stage 2: the neighbour table
    bounds = nbm.plan_bounds()
    make = lambda: nbm.neighbours(index, other, count, ids, df, args.k, "both", "dice")     # noqa: E731
    make()                                                                                  # warm-up
    table, t_nb = _timed(make, args.reps)
    kernels = _kernels(lib, make)
    E = 2 * nnz
    deg = torch.bincount(torch.cat([torch.searchsorted(ids.to(torch.int64), index.to(torch.int64)),
                                    torch.searchsorted(ids.to(torch.int64), other.to(torch.int64))]), minlength=u)
    classes = [int(((deg > lo) & (deg <= hi)).sum()) for lo, hi in zip([-1] + bounds, bounds + [1 << 62])]
    class_entries = [int(deg[(deg > lo) & (deg <= hi)].sum()) for lo, hi in zip([-1] + bounds, bounds + [1 << 62])]
    kept = int(table.lengths.sum())
    # algorithmic bytes: degree reads the two id columns and writes the two row columns; fill reads id, row and count
    # columns and writes a key and a count per listed entry; the select reads those lists once and writes the padded
    # table (three [u, k] planes) and the lengths
    stage_bytes = 16 * nnz + (20 * nnz + 12 * E) + 12 * E + 12 * u * args.k + 4 * u
    wave_bytes = 12 * (class_entries[0] + class_entries[1]) + 12 * min(kept, class_entries[0] + class_entries[1])
    best = min(t_nb)
    wave_ms = kernels.get("nb_select_wave", {}).get("ms")
    rec2 = {"bench": "neighbours", "stage": "neighbours", "k": args.k, "orientation": "both", "score": "dice",
            "rows": u, "entries": E, "kept": kept, "plan_bounds": bounds, "rows_per_class": classes,
            "entries_per_class": class_entries, "longest_row": int(deg.max()), "reps": args.reps,
            "ms": round(best * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in t_nb], "rows_per_s": round(u / best),
            "entries_per_s": round(E / best), "algorithmic_bytes": stage_bytes,
            "bytes_per_s": round(stage_bytes / best), "fraction_of_8TBps": round(stage_bytes / best / HBM, 4),
            "kernels_ms": kernels,
            "select_wave": {"list_and_output_bytes": wave_bytes, "ms": wave_ms,
                            "fraction_of_8TBps": round(wave_bytes / (wave_ms * 1e-3) / HBM, 4) if wave_ms else None}}

    # the torch restatement, same session, same GPU
    ref = lambda: torch_neighbours(index, other, count, ids, df, args.k)                     # noqa: E731
    ref()
    (r_nb, r_sc, r_len), t_ref = _timed(ref, args.reps)
    same = bool(torch.equal(r_nb, table.neighbours) and torch.equal(r_sc, table.scores) and
                torch.equal(r_len, table.lengths))
    rec2["torch_restatement"] = {"ms": round(min(t_ref) * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in t_ref],
                                 "equal_to_kernel_table": same, "kernel_speedup": round(min(t_ref) / best, 2)}
    print(json.dumps(rec2))
    del r_nb, r_sc, r_len

    # stage 3: recommend
    q_rng = np.random.default_rng(1)
    history = torch.from_numpy(indices[q_rng.integers(0, indices.size, args.queries * args.history)]).to(dev)
    q_off = torch.arange(args.queries + 1, dtype=torch.int64, device=dev) * args.history
    rec = lambda: nbm.recommend(table, history, q_off, args.rec_k)                           # noqa: E731
    rec()
    (r_ids, r_scores, r_lengths), t_rec = _timed(rec, max(args.reps, 20))
    k_rec = _kernels(lib, rec)
    entries = args.queries * args.history * args.k
    rec_bytes = 4 * args.queries * args.history + 8 * entries + 8 * args.queries * args.rec_k + 4 * args.queries
    best = min(t_rec)
    print(json.dumps({"bench": "neighbours", "stage": "recommend", "queries": args.queries, "history": args.history,
                      "table_width": args.k, "k": args.rec_k, "entries": entries,
                      "mean_length": round(float(r_lengths.float().mean()), 2), "reps": len(t_rec),
                      "ms": round(best * 1e3, 3), "ms_median": round(float(np.median(t_rec)) * 1e3, 3),
                      "queries_per_s": round(args.queries / best), "entries_per_s": round(entries / best),
                      "algorithmic_bytes": rec_bytes, "bytes_per_s": round(rec_bytes / best),
                      "fraction_of_8TBps": round(rec_bytes / best / HBM, 4), "kernels_ms": k_rec}))


if __name__ == "__main__":
    main()

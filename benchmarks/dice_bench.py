"""Dice (set co-occurrence) builder on one MI355X: documents/s and pair increments/s of DiceBuilder.add + finalize on
synthetic Zipf id sets -- set sizes around 20 with a thin tail up to the cap -- beside the CPU restatement of the same rule
(tests/_dice_ref.py: pure-Python dictionary work, what the reference's Spark workers run per partition) on a prefix of
the same corpus.  Prints one JSON line.  The yardstick is benchmarks/cooccur_bench.py's window hits/s, run in the same
session on the same box: the same table under the same atomics.

    python benchmarks/dice_bench.py [--docs 1000000] [--vocab 200000] [--mean 20] [--reps 3] [--cpu_docs 3000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _corpus(rng, ndocs, V, mean, a, tail, cap):
    """Set sizes: Poisson(mean); one document in `tail` draws 64 x Pareto(1) instead, cut at the cap."""
    n = rng.poisson(mean, ndocs)
    heavy = rng.random(ndocs) < 1.0 / tail
    n[heavy] = np.minimum(cap, (64 * (1 + rng.pareto(1.0, int(heavy.sum())))).astype(np.int64))
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    indices = ((rng.zipf(a, int(off[-1])) - 1) % V).astype(np.int32)
    return indices, off


def _pair_increments(indices, off, V):
    """Sum over documents of u (u - 1) / 2 with u = the document's distinct ids: what the kernels add to pair keys."""
    doc = np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off))
    u = np.bincount(np.unique(doc * V + indices) // V, minlength=off.size - 1)
    return int((u * (u - 1) // 2).sum()), int(u.sum())


def _kernel_times(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.esr_kernel_timing_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, total, mn, mx = line.split("\t")
        out[name] = {"calls": int(calls), "ms": round(float(total), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--mean", type=int, default=20)
    ap.add_argument("--tail", type=int, default=2000, help="one document in this many is drawn from the heavy tail")
    ap.add_argument("--zipf", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu_docs", type=int, default=3000)
    args = ap.parse_args()
    from _dice_ref import ref_dice
    from esrecsys_amd import _lib
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC, DiceBuilder
    dev = torch.device("cuda", 0)
    indices, off = _corpus(np.random.default_rng(0), args.docs, args.vocab, args.mean, args.zipf, args.tail, MAX_DOC)
    sizes = np.diff(off)
    increments, df_increments = _pair_increments(indices, off, args.vocab)
    d_indices, d_off = torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev)
    DiceBuilder(capacity=1 << 10, device=dev).add(indices[:off[3]], off[:4]).finalize()   # warm-up
    torch.cuda.synchronize()
    add_s, fin_s, grow_s = [], [], []
    nnz = cap = rehashes = launches = 0
    for capacity, bucket in ((1 << 20, grow_s), (None, add_s)):
        # first from the default capacity (the table grows by rehash on the way), then pre-sized: no rehash
        for _ in range(args.reps):
            b = DiceBuilder(capacity=capacity or cap, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.add(d_indices, d_off)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = b.finalize()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            bucket.append(t1 - t0)
            if capacity is None:
                fin_s.append(t2 - t1)
            nnz, cap, rehashes, launches = b.nnz, b.capacity, max(rehashes, b.rehashes), b.launches
            del b, out
    lib = _lib.load()
    lib.esr_kernel_timing(1)
    b = DiceBuilder(capacity=cap, device=dev)
    b.add(d_indices, d_off).finalize()
    torch.cuda.synchronize()
    kernels = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    del b
    # the CPU restatement on a prefix of the documents
    ndocs_cpu = min(args.cpu_docs, args.docs)
    docs = [indices[off[d]:off[d + 1]] for d in range(ndocs_cpu)]
    t0 = time.perf_counter()
    ref_dice(docs)
    cpu_s = time.perf_counter() - t0
    cpu_inc = _pair_increments(indices[:off[ndocs_cpu]], off[:ndocs_cpu + 1], args.vocab)[0]
    add, fin, grow = min(add_s), min(fin_s), min(grow_s)
    print(json.dumps({
        "bench": "dice", "docs": int(args.docs), "ids": int(off[-1]), "vocab": args.vocab, "zipf_a": args.zipf,
        "set_size_mean": round(float(sizes.mean()), 2), "set_size_max": int(sizes.max()),
        "docs_above_64_ids": int((sizes > 64).sum()), "pair_increments": increments, "df_increments": df_increments,
        "nnz": nnz, "capacity": cap, "launches": launches, "reps": args.reps,
        "add_ms": round(add * 1e3, 3), "add_ms_all": [round(x * 1e3, 3) for x in add_s],
        "add_growing_ms": round(grow * 1e3, 3), "rehashes_when_growing": rehashes,
        "finalize_ms": round(fin * 1e3, 3), "finalize_ms_all": [round(x * 1e3, 3) for x in fin_s],
        "docs_per_s": round(args.docs / (add + fin)), "pair_increments_per_s": round(increments / (add + fin)),
        "add_docs_per_s": round(args.docs / add), "add_pair_increments_per_s": round(increments / add),
        "kernels": kernels,
        "cpu_restatement": {"docs": ndocs_cpu, "pair_increments": cpu_inc, "s": round(cpu_s, 3),
                            "docs_per_s": round(ndocs_cpu / cpu_s), "pair_increments_per_s": round(cpu_inc / cpu_s)},
        "speedup_vs_cpu_restatement": round((increments / (add + fin)) / (cpu_inc / cpu_s), 1)}))


if __name__ == "__main__":
    main()

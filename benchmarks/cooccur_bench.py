"""Co-occurrence builder on one MI355X: tokens/s and window pairs/s of CooccurrenceBuilder.add + finalize on a synthetic
Zipf corpus, beside the CPU restatement of the same rule (tests/_cooccur_ref.py: pure-Python dictionary work, what the
reference's Spark workers run per partition) on a prefix of the same corpus.  Prints one JSON line.

    python benchmarks/cooccur_bench.py [--tokens 8000000] [--vocab 200000] [--window 10] [--reps 3] [--cpu_tokens 40000]
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


def _corpus(rng, n_tokens, V, doc_len, a):
    tokens = ((rng.zipf(a, n_tokens) - 1) % V).astype(np.int32)
    lens = rng.integers(doc_len // 2, doc_len * 3 // 2, n_tokens // doc_len + 2)
    off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n_tokens)
    off = off[:int(np.searchsorted(off, n_tokens)) + 1].astype(np.int64)
    return tokens, off


def _window_hits(off, W):
    """Position pairs the kernel visits: per document of n tokens, sum over q of min(q, W)."""
    n = np.diff(off)
    short = n * (n - 1) // 2
    long_ = W * (W + 1) // 2 + (n - 1 - W) * W
    return int(np.where(n <= W, short, long_).sum())


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
    ap.add_argument("--tokens", type=int, default=8_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--doc_len", type=int, default=1000)
    ap.add_argument("--zipf", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu_tokens", type=int, default=40_000)
    args = ap.parse_args()
    from _cooccur_ref import ref_exact
    from esrecsys_amd import _lib
    from esrecsys_amd.wikipedia.make_cooccurrence import CooccurrenceBuilder
    dev = torch.device("cuda", 0)
    W = args.window
    tokens, off = _corpus(np.random.default_rng(0), args.tokens, args.vocab, args.doc_len, args.zipf)
    d_tokens, d_off = torch.from_numpy(tokens).to(dev), torch.from_numpy(off).to(dev)
    hits = _window_hits(off, W)
    CooccurrenceBuilder(W, capacity=1 << 10, device=dev).add(tokens[:off[3]], off[:4]).finalize()   # warm-up
    torch.cuda.synchronize()
    add_s, fin_s, grow_s = [], [], []
    nnz = cap = rehashes = 0
    for capacity, bucket in ((1 << 20, grow_s), (None, add_s)):
        # first from the default capacity (the table grows by rehash on the way), then pre-sized: no rehash
        for _ in range(args.reps):
            b = CooccurrenceBuilder(W, capacity=capacity or cap, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.add(d_tokens, d_off)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = b.finalize()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            bucket.append(t1 - t0)
            if capacity is None:
                fin_s.append(t2 - t1)
            nnz, cap, rehashes = b.nnz, b.capacity, max(rehashes, b.rehashes)
            del b, out
    lib = _lib.load()
    lib.esr_kernel_timing(1)
    b = CooccurrenceBuilder(W, capacity=cap, device=dev)
    b.add(d_tokens, d_off).finalize()
    torch.cuda.synchronize()
    kernels = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    # the CPU restatement on a prefix (whole documents)
    ndocs_cpu = max(1, int(np.searchsorted(off, args.cpu_tokens)))
    docs = [tokens[off[d]:off[d + 1]] for d in range(ndocs_cpu)]
    t0 = time.perf_counter()
    ref_exact(docs, W)
    cpu_s = time.perf_counter() - t0
    cpu_tokens = int(off[ndocs_cpu])
    add, fin, grow = min(add_s), min(fin_s), min(grow_s)
    print(json.dumps({
        "bench": "cooccur", "tokens": int(args.tokens), "docs": int(off.size - 1), "vocab": args.vocab, "window": W,
        "zipf_a": args.zipf, "window_hits": hits, "nnz": nnz, "capacity": cap, "reps": args.reps,
        "add_ms": round(add * 1e3, 3), "add_ms_all": [round(x * 1e3, 3) for x in add_s],
        "add_growing_ms": round(grow * 1e3, 3), "rehashes_when_growing": rehashes,
        "finalize_ms": round(fin * 1e3, 3), "finalize_ms_all": [round(x * 1e3, 3) for x in fin_s],
        "tokens_per_s": round(args.tokens / (add + fin)), "window_hits_per_s": round(hits / (add + fin)),
        "add_tokens_per_s": round(args.tokens / add), "add_window_hits_per_s": round(hits / add),
        "kernels": kernels,
        "cpu_restatement": {"tokens": cpu_tokens, "s": round(cpu_s, 3), "tokens_per_s": round(cpu_tokens / cpu_s)},
        "speedup_vs_cpu_restatement": round((args.tokens / (add + fin)) / (cpu_tokens / cpu_s), 1)}))


if __name__ == "__main__":
    main()

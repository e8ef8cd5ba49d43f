"""Term stages on one MI355X: tokens/s of the three id-level legs in front of the co-occurrence builder, on a synthetic
Zipf corpus over sparse provisional ids, each beside the CPU restatement of the same rule (tests/_terms_ref.py:
pure-Python dictionary work, what the reference's Spark workers run per partition) on a prefix of the same corpus.

    statistics   TermStatsBuilder.add + finalize
    embedding    Dictionary.embedding_indices
    tfidf        TfidfBuilder.transform

Prints one JSON line per leg.

    python benchmarks/terms_bench.py [--tokens 8000000] [--vocab 200000] [--reps 3] [--cpu_tokens 200000]
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
    """The corpus of cooccur_bench.py, its ids spread over [0, 2^31) (an odd multiplier: a bijection)."""
    dense = (rng.zipf(a, n_tokens) - 1) % V
    tokens = ((dense.astype(np.int64) * 2654435761 + 12345) % (1 << 31)).astype(np.int32)
    lens = rng.integers(doc_len // 2, doc_len * 3 // 2, n_tokens // doc_len + 2)
    off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n_tokens)
    off = off[:int(np.searchsorted(off, n_tokens)) + 1].astype(np.int64)
    return tokens, off


def _kernel_times(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.esr_kernel_timing_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, total, mn, mx = line.split("\t")
        out[name] = {"calls": int(calls), "ms": round(float(total), 4)}
    return out


def _timed(fn, reps):
    out, best = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best.append(time.perf_counter() - t0)
    return out, best


def _traced(lib, fn):
    lib.esr_kernel_timing(1)
    fn()
    torch.cuda.synchronize()
    kernels = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=8_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc_len", type=int, default=1000)
    ap.add_argument("--zipf", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu_tokens", type=int, default=200_000)
    ap.add_argument("--min_frequency", type=int, default=20)
    ap.add_argument("--max_tokens_per_launch", type=int, default=1 << 21)
    args = ap.parse_args()
    import _terms_ref as tr
    from esrecsys_amd import _lib
    from esrecsys_amd.wikipedia.count_terms import TfidfBuilder
    from esrecsys_amd.wikipedia.make_dictionary import TermStatsBuilder, make_token_dictionary
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    tokens, off = _corpus(np.random.default_rng(0), args.tokens, args.vocab, args.doc_len, args.zipf)
    d_tokens, d_off = torch.from_numpy(tokens).to(dev), torch.from_numpy(off).to(dev)
    common = {"tokens": int(args.tokens), "docs": int(off.size - 1), "vocab": args.vocab, "zipf_a": args.zipf,
              "reps": args.reps, "max_tokens_per_launch": args.max_tokens_per_launch}
    # the CPU restatements on a prefix (whole documents)
    ndocs_cpu = max(1, int(np.searchsorted(off, args.cpu_tokens)))
    cpu_docs = [tokens[off[d]:off[d + 1]] for d in range(ndocs_cpu)]
    cpu_tokens = int(off[ndocs_cpu])

    def cpu_leg(fn):
        t0 = time.perf_counter()
        out = fn()
        s = time.perf_counter() - t0
        return out, {"tokens": cpu_tokens, "s": round(s, 3), "tokens_per_s": round(cpu_tokens / s)}

    def stats_leg(capacity=1 << 20):
        b = TermStatsBuilder(capacity=capacity, device=dev, max_tokens_per_launch=args.max_tokens_per_launch)
        out = b.add(d_tokens, d_off).finalize()
        stats_leg.builder = b
        return out

    TermStatsBuilder(capacity=1 << 10, device=dev).add(tokens[:off[3]], off[:4]).finalize()   # warm-up
    stats, s = _timed(stats_leg, args.reps)
    b = stats_leg.builder
    cpu_stats, cpu = cpu_leg(lambda: tr.ref_stats(cpu_docs))
    print(json.dumps(dict(common, bench="terms_statistics", ids=int(stats[0].numel()), capacity=b.capacity,
                          rehashes=b.rehashes, launches=b.launches, ms=round(min(s) * 1e3, 3),
                          ms_all=[round(x * 1e3, 3) for x in s], tokens_per_s=round(args.tokens / min(s)),
                          kernels=_traced(lib, stats_leg), cpu_restatement=cpu,
                          speedup_vs_cpu_restatement=round(args.tokens / min(s) / cpu["tokens_per_s"], 1))))

    dictionary = make_token_dictionary(*stats, min_frequency=args.min_frequency)
    dictionary.embedding_indices(d_tokens[:1000])                                           # builds the lookup table
    emb, s = _timed(lambda: dictionary.embedding_indices(d_tokens), args.reps)
    cpu_dict = tr.ref_dictionary(*cpu_stats, min_frequency=2)
    _, cpu = cpu_leg(lambda: tr.ref_embedding(np.concatenate(cpu_docs), cpu_dict[0]))
    inside = float((emb <= dictionary.size).float().mean())
    print(json.dumps(dict(common, bench="terms_embedding_indices", dictionary_size=dictionary.size,
                          inside_dictionary=round(inside, 4), ms=round(min(s) * 1e3, 3),
                          ms_all=[round(x * 1e3, 3) for x in s], tokens_per_s=round(args.tokens / min(s)),
                          kernels=_traced(lib, lambda: dictionary.embedding_indices(d_tokens)), cpu_restatement=cpu,
                          speedup_vs_cpu_restatement=round(args.tokens / min(s) / cpu["tokens_per_s"], 1))))

    stop = set(dictionary.ids[:20].tolist())
    tfidf = TfidfBuilder(dictionary, stopwords=stop, device=dev, max_tokens_per_launch=args.max_tokens_per_launch)
    tfidf.transform(tokens[:off[3]], off[:4])                                               # warm-up, lookup table
    launches0 = tfidf.launches
    out, s = _timed(lambda: tfidf.transform(d_tokens, d_off), args.reps)
    _, cpu = cpu_leg(lambda: tr.ref_sparse_docs(cpu_docs, cpu_dict[0], cpu_dict[2], int(cpu_dict[2].max()),
                                                set(cpu_dict[0][:20].tolist())))
    print(json.dumps(dict(common, bench="terms_tfidf", dictionary_size=dictionary.size, stopwords=len(stop),
                          nnz=int(out[1].numel()), launches_per_transform=(tfidf.launches - launches0) // args.reps,
                          ms=round(min(s) * 1e3, 3), ms_all=[round(x * 1e3, 3) for x in s],
                          tokens_per_s=round(args.tokens / min(s)),
                          kernels=_traced(lib, lambda: tfidf.transform(d_tokens, d_off)), cpu_restatement=cpu,
                          speedup_vs_cpu_restatement=round(args.tokens / min(s) / cpu["tokens_per_s"], 1))))


if __name__ == "__main__":
    main()

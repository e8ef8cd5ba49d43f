"""Explicit ratings on one MI355X: UserSimilarityBuilder.add + finalize, neighbours() on the result and UserKnn.recommend
for 8192 users, on a synthetic corpus -- items of Zipf-Mandelbrot popularity (p(i) ~ 1 / (i + 1 + q)^a), half-star ratings,
sized so that the pair increments are of the order of benchmarks/dice_bench.py's -- beside a plain-torch restatement of the
similarity job in the same session (pairs expanded by index arithmetic, one sort of the keys, segment sums in int64, the
same fp64 expression), whose table must equal the builder's bit for bit.  Prints one JSON line.

    python benchmarks/ratings_bench.py [--users 30000] [--items 20000] [--per_user 14] [--reps 3]
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


def _corpus(rng, users, items, per_user, a, q):
    """One rating per (user, item): per_user draws per user from the popularity law, repeats dropped."""
    w = 1.0 / np.arange(1 + q, items + 1 + q, dtype=np.float64) ** a
    item = rng.choice(items, users * per_user, p=w / w.sum())
    user = np.repeat(np.arange(users, dtype=np.int64), per_user)
    key = np.unique(user * items + item)
    user, item = key // items, key % items
    rating = rng.integers(1, 11, key.size) / 2.0
    return user.astype(np.int32), item.astype(np.int32), rating


def _kernel_times(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.esr_kernel_timing_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, total, mn, mx = line.split("\t")
        out[name] = {"calls": int(calls), "ms": round(float(total), 4)}
    return out


def torch_similarity(user, item, dev):
    """The similarity job in plain torch: (index, other, sim, overlap) ascending by (index, other), flat entries dropped."""
    order = torch.sort((item.to(torch.int64) << 32) | user.to(torch.int64)).indices
    u, d = user[order].to(torch.int64), dev[order].to(torch.int64)
    _ids, n = torch.unique_consecutive(item[order], return_counts=True)
    start = torch.cumsum(n, 0) - n
    pairs = n * (n - 1) // 2
    it = torch.repeat_interleave(torch.arange(n.numel(), device=n.device), pairs)
    local = torch.arange(int(pairs.sum()), device=n.device) - torch.repeat_interleave(torch.cumsum(pairs, 0) - pairs, pairs)
    # pair x of a triangle, column by column: x = q (q - 1) / 2 + p with p < q
    q = ((1.0 + torch.sqrt(1.0 + 8.0 * local.to(torch.float64))) * 0.5).to(torch.int64)
    q = torch.where(q * (q - 1) // 2 > local, q - 1, q)
    q = torch.where((q + 1) * q // 2 <= local, q + 1, q)
    p = local - q * (q - 1) // 2
    a, b = start[it] + p, start[it] + q
    key, by_key = torch.sort((u[a] << 32) | u[b])
    da, db = d[a][by_key], d[b][by_key]
    uniq, inverse, overlap = torch.unique_consecutive(key, return_inverse=True, return_counts=True)
    zeros = lambda: torch.zeros(uniq.numel(), dtype=torch.int64, device=key.device)  # noqa: E731
    P, Qa, Qb = zeros().index_add_(0, inverse, da * db), zeros().index_add_(0, inverse, da * da), \
        zeros().index_add_(0, inverse, db * db)
    keep = (Qa != 0) & (Qb != 0)
    sim = (P.to(torch.float64) / (torch.sqrt(Qa.to(torch.float64)) * torch.sqrt(Qb.to(torch.float64)))).to(torch.float32)
    return ((uniq >> 32)[keep].to(torch.int32), (uniq & 0xFFFFFFFF)[keep].to(torch.int32), sim[keep],
            overlap[keep].to(torch.int32))


def _best(fn, reps):
    times, out = [], None
    for _ in range(reps):
        del out
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=30000)
    ap.add_argument("--items", type=int, default=20000)
    ap.add_argument("--per_user", type=int, default=14)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--shift", type=float, default=20.0)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from esrecsys_amd import _lib, ops
    from esrecsys_amd import ratings as rt
    from esrecsys_amd.wikipedia.neighbours import neighbours
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    user, item, rating = _corpus(rng, args.users, args.items, args.per_user, args.zipf, args.shift)
    n_item = np.bincount(item, minlength=args.items).astype(np.int64)
    increments = int((n_item * (n_item - 1) // 2).sum())
    tiles = int(rt.UserSimilarityBuilder.tiles_of(n_item, ops.usersim_tile()).sum())
    d_user, d_item = torch.from_numpy(user).to(dev), torch.from_numpy(item).to(dev)
    d_rating = torch.from_numpy(rating).to(dev)
    users, mean, d = rt.rating_deviations(d_user, d_rating)
    rt.UserSimilarityBuilder(capacity=1 << 10, device=dev).add(user[:64], item[:64], d[:64]).finalize()   # warm-up
    torch.cuda.synchronize()
    cap = 1 << 20
    grow_s, add_s, fin_s = [], [], []
    out = b = None
    for presized in (False, True):
        # first from the default capacity (the table grows by rehash on the way), then pre-sized: no rehash
        for _ in range(args.reps):
            del out, b
            b = rt.UserSimilarityBuilder(capacity=cap, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b.add(d_user, d_item, d)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = b.finalize()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            (add_s if presized else grow_s).append(t1 - t0)
            if presized:
                fin_s.append(t2 - t1)
        rehashes = b.rehashes if not presized else rehashes
        cap = b.capacity
    index, other, sim, overlap = out
    launches, flat = b.launches, b.dropped_flat
    lib = _lib.load()
    lib.esr_kernel_timing(1)
    kb = rt.UserSimilarityBuilder(capacity=cap, device=dev)
    kb.add(d_user, d_item, d).finalize()
    torch.cuda.synchronize()
    kernels = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    del kb, b
    torch_s, ref = _best(lambda: torch_similarity(d_user, d_item, d), args.reps)
    for name, g, w in zip(("index", "other", "sim", "overlap"), out, ref):
        assert torch.equal(g, w), "the torch restatement's %s differs from the builder's" % name
    del ref
    nb_s, table = _best(lambda: neighbours(index, other, sim, users, None, args.k, "both", "count"), args.reps)
    model = rt.UserKnn(table, d_user, d_item, d_rating, users, mean)
    queries = torch.from_numpy(rng.choice(args.users, min(args.queries, args.users), replace=False).astype(np.int32)).to(dev)
    rec_s, rec = _best(lambda: model.recommend(queries, 500), max(args.reps, 10))
    gathered = model.gathered(queries)
    add, fin, grow, tsim = min(add_s), min(fin_s), min(grow_s), min(torch_s)
    ms = lambda xs: [round(x * 1e3, 3) for x in xs]  # noqa: E731
    print(json.dumps({
        "bench": "ratings", "users": args.users, "items": args.items, "ratings": int(user.size), "zipf_a": args.zipf,
        "shift": args.shift, "raters_max": int(n_item.max()), "raters_mean": round(float(n_item[n_item > 0].mean()), 2),
        "pair_increments": increments, "tiles": tiles, "tile": ops.usersim_tile(), "nnz": int(index.numel()),
        "dropped_flat": int(flat), "capacity": cap, "launches": launches, "reps": args.reps,
        "add_ms": round(add * 1e3, 3), "add_ms_all": ms(add_s), "add_growing_ms": round(grow * 1e3, 3),
        "rehashes_when_growing": rehashes, "finalize_ms": round(fin * 1e3, 3), "finalize_ms_all": ms(fin_s),
        "pair_increments_per_s": round(increments / (add + fin)), "add_pair_increments_per_s": round(increments / add),
        "kernels": kernels,
        "torch_restatement_ms": round(tsim * 1e3, 3), "torch_restatement_ms_all": ms(torch_s), "tables_equal": True,
        "torch_over_kernel_path": round(tsim / (add + fin), 3),
        "neighbours_ms": round(min(nb_s) * 1e3, 3), "neighbours_ms_all": ms(nb_s), "k": args.k,
        "recommend_queries": int(queries.numel()), "recommend_k": 500, "recommend_ms": round(min(rec_s) * 1e3, 3),
        "recommend_ms_all": ms(rec_s), "recommend_gathered_mean": round(float(gathered.float().mean()), 2),
        "recommend_gathered_max": int(gathered.max()), "recommended_mean": round(float(rec[2].float().mean()), 2)}))


if __name__ == "__main__":
    main()

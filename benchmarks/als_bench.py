"""ALS on explicit ratings on one MI355X: the user half-sweep, the item half-sweep and the whole sweep of
esrecsys_amd/factorization.py at ranks 32 and 64, on the ratings benchmark's corpus (benchmarks/ratings_bench.py: 30 000
users, 20 000 Zipf-Mandelbrot items, 14 draws per user) and on a larger synthetic one generated on the device (140 000
users, 27 000 items of the same law, about 20 M ratings) -- beside a plain-torch restatement of the same half-sweep in the
same session (chunked ``index_add_`` of outer products, ``torch.linalg.cholesky`` + ``cholesky_solve``), with both compared
against the same restatement in fp64.  Reported context: RMSE and recall@10 on a leave-last-out split.  Prints one JSON line.

    python benchmarks/als_bench.py [--reps 5] [--inner 10] [--skip_large] [--skip_torch]
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
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

HBM_BYTES_PER_S = 8.0e12          # MI355X HBM3E peak
F32_MATRIX_FLOPS = 157.3e12       # v_mfma_f32_32x32x2_f32 peak
ULP32 = 2.0 ** -23


def device_corpus(users, items, per_user, a, q, dev, seed):
    """The popularity law of ratings_bench._corpus drawn on the device by inverse CDF; repeats of a pair dropped; a
    timestamp per rating (a random order inside a user) for the leave-last-out split."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    w = 1.0 / torch.arange(1 + q, items + 1 + q, dtype=torch.float64, device=dev) ** a
    cdf = torch.cumsum(w / w.sum(), 0)
    draws = torch.rand(users * per_user, generator=gen, device=dev, dtype=torch.float64)
    item = torch.searchsorted(cdf, draws).clamp(max=items - 1)
    user = torch.arange(users, device=dev).repeat_interleave(per_user)
    key = torch.unique(user * items + item)
    user, item = key // items, key % items
    rating = torch.randint(1, 11, (key.numel(),), generator=gen, device=dev).to(torch.float64) / 2.0
    tstamp = torch.rand(key.numel(), generator=gen, device=dev)
    return user.to(torch.int32), item.to(torch.int32), rating, tstamp


def _kernel_times(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.esr_kernel_timing_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, total, mn, mx = line.split("\t")
        out[name] = {"calls": int(calls), "ms": round(float(total), 4)}
    return out


def _windows(fn, reps, inner):
    """`reps` windows of `inner` calls each, a synchronise at both ends: seconds per call of every window."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / inner)
    return out


def torch_half_sweep(Y, offsets, cols, targets, reg, weighted, dtype, slab):
    """The half-sweep in plain torch: the Gram matrices and right-hand sides by index_add_ of outer products over slabs of
    `slab` ratings, then a batched Cholesky solve.  (Atomic adds: its sums have no fixed order.)"""
    dev = Y.device
    n_rows, rank = offsets.numel() - 1, Y.shape[1]
    counts = offsets[1:] - offsets[:-1]
    row = torch.repeat_interleave(torch.arange(n_rows, device=dev), counts)
    Yd = Y.to(dtype)
    G = torch.zeros((n_rows, rank, rank), dtype=dtype, device=dev)
    b = torch.zeros((n_rows, rank), dtype=dtype, device=dev)
    for s in range(0, cols.numel(), slab):
        y = Yd[cols[s:s + slab].to(torch.int64)]
        G.index_add_(0, row[s:s + slab], y[:, :, None] * y[:, None, :])
        b.index_add_(0, row[s:s + slab], y * targets[s:s + slab].to(dtype)[:, None])
        del y
    lam = torch.full((n_rows,), float(np.float32(reg)), dtype=dtype, device=dev)
    if weighted:
        lam = lam * counts.to(dtype)
    lam = torch.where(counts > 0, lam, torch.ones_like(lam))       # an empty row: I x = 0
    G.diagonal(dim1=1, dim2=2).add_(lam[:, None])
    L = torch.linalg.cholesky(G)
    del G
    return torch.cholesky_solve(b[:, :, None], L)[:, :, 0]


def row_errors(x, x64):
    """max|x - x64| / max|x64| per row (0 for an all-zero reference row that is matched)."""
    scale = x64.abs().amax(1).clamp(min=1e-300)
    return ((x.to(torch.float64) - x64).abs().amax(1) / scale)


def bench_config(name, user, item, rating, rank, args, dev, lib, with_torch):
    from esrecsys_amd import factorization as fz
    from esrecsys_amd import ops
    rec = {"corpus": name, "rank": rank}
    t0 = time.perf_counter()
    model = fz.RatingsALS(user, item, rating, rank=rank, reg=0.1, device=dev)
    torch.cuda.synchronize()
    nnz, nu, ni = model.nnz, int(model.users.numel()), int(model.items.numel())
    rec.update({"ratings": nnz, "users": nu, "items": ni, "build_ms": round((time.perf_counter() - t0) * 1e3, 1),
                "longest_user_row": int(np.diff(model._user_offsets).max()),
                "longest_item_row": int(np.diff(model._item_offsets).max())})
    model.sweep()                                  # warm-up: code objects, the LDS limit, the allocator
    model.sweep()
    tu = _windows(model.solve_users, args.reps, args.inner)
    ti = _windows(model.solve_items, args.reps, args.inner)
    ts = _windows(model.sweep, args.reps, args.inner)
    u, i, s = min(tu), min(ti), min(ts)
    ms = lambda xs: [round(x * 1e3, 4) for x in xs]  # noqa: E731
    rec.update({"user_half_sweep_ms": round(u * 1e3, 4), "user_half_sweep_ms_all": ms(tu),
                "item_half_sweep_ms": round(i * 1e3, 4), "item_half_sweep_ms_all": ms(ti),
                "sweep_ms": round(s * 1e3, 4), "sweep_ms_all": ms(ts),
                "ratings_per_s_sweep": round(2 * nnz / s),
                "gather_bytes_per_half_sweep": nnz * rank * 4, "gram_flops_per_half_sweep": 2 * nnz * rank * rank})
    for side, t in (("user", u), ("item", i)):
        rec[side + "_fraction_of_hbm_peak"] = round(nnz * rank * 4 / t / HBM_BYTES_PER_S, 5)
        rec[side + "_fraction_of_f32_matrix_peak"] = round(2 * nnz * rank * rank / t / F32_MATRIX_FLOPS, 5)
    lib.esr_kernel_timing(1)
    model.sweep()
    torch.cuda.synchronize()
    rec["kernels_one_sweep"] = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    if with_torch:
        slab = max(1 << 12, (1 << 28) // (rank * rank))          # about 1 GiB of f32 outer products per slab
        for side, Y, off, cols, tg, solve, out in (
                ("user", model.item_factors, model._user_offsets, model._row_ipos, model._targets, model.solve_users,
                 model.user_factors),
                ("item", model.user_factors, model._item_offsets, model._col_upos, model._targets_by_item,
                 model.solve_items, model.item_factors)):
            off_d = torch.from_numpy(off).to(dev)
            Y0 = Y.clone()
            solve()                                          # the kernel's rows from Y0
            got = out.clone()
            torch_half_sweep(Y0[:64], off_d[:9].clamp(max=8), cols[:8].clamp(max=63), tg[:8], 0.1, True, torch.float32, slab)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x32 = torch_half_sweep(Y0, off_d, cols, tg, 0.1, True, torch.float32, slab)
            torch.cuda.synchronize()
            t32 = time.perf_counter() - t0
            x64 = torch_half_sweep(Y0, off_d, cols, tg, 0.1, True, torch.float64, slab // 2)
            ek, et = row_errors(got, x64), row_errors(x32, x64)
            within = bool(float(ek.max()) <= 4 * float(et.max()) + 8 * ULP32)
            rec[side + "_torch_restatement_ms"] = round(t32 * 1e3, 3)
            rec[side + "_torch_over_kernel_path"] = round(t32 / (u if side == "user" else i), 2)
            rec[side + "_kernel_error_vs_fp64_max"] = float(ek.max())
            rec[side + "_torch_f32_error_vs_fp64_max"] = float(et.max())
            rec[side + "_rows_within_4x_plus_8ulp_of_torch_f32"] = round(float((ek <= 4 * et + 8 * ULP32).double().mean()), 6)
            rec[side + "_equal_within_tolerance"] = within
            assert within, "%s rank %d %s: kernel error %g against torch f32 error %g" % (name, rank, side, float(ek.max()),
                                                                                        float(et.max()))
            del x32, x64, got, Y0, ek, et
            torch.cuda.empty_cache()
    rec["chunk"] = ops.als_geometry()[0]
    del model
    return rec


def quality(name, user, item, rating, tstamp, rank, sweeps, dev):
    """Leave-last-out: the latest rating of every user with at least two is held out; RMSE on the held-out pairs and
    recall@10 of ``recommend`` for up to 8192 of those users."""
    from esrecsys_amd import evaluate
    from esrecsys_amd import factorization as fz
    order = torch.sort((user.to(torch.int64) << 32) | (tstamp * (2 ** 31 - 1)).to(torch.int64)).indices
    u_s = user[order]
    last = torch.ones(u_s.numel(), dtype=torch.bool, device=dev)
    last[:-1] = u_s[1:] != u_s[:-1]
    first = torch.ones_like(last)
    first[1:] = u_s[1:] != u_s[:-1]
    held = last & ~first                                            # a user's only rating stays in training
    tr, te = order[~held], order[held]
    model = fz.RatingsALS(user[tr], item[tr], rating[tr], rank=rank, reg=0.1, device=dev)
    history = model.fit(sweeps=sweeps)
    q = te[:8192]
    ids, _, lens = model.recommend(user[q], k=10)
    m = evaluate.ranking_metrics(ids, lens, item[q].to(torch.int32), np.arange(q.numel() + 1, dtype=np.int64), ks=(10,))
    return {"corpus": name, "rank": rank, "sweeps": sweeps, "train_ratings": int(tr.numel()), "held_out": int(te.numel()),
            "objective_first": history[0], "objective_last": history[-1],
            "objective_non_increasing": bool(all(b <= a for a, b in zip(history, history[1:]))),
            "train_rmse": round(model.rmse(user[tr], item[tr], rating[tr]), 5),
            "held_out_rmse": round(model.rmse(user[te], item[te], rating[te]), 5),
            "held_out_rmse_of_user_mean": round(float(torch.sqrt(((model.user_mean[model._positions(user[te], model.users)
                                                                                   .to(torch.int64)] - rating[te]) ** 2)
                                                                 .mean())), 5),
            "recall_at_10": float(m.mean()["recall"][0]), "recommend_queries": int(q.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--quality_sweeps", type=int, default=5)
    ap.add_argument("--skip_large", action="store_true")
    ap.add_argument("--skip_torch", action="store_true")
    args = ap.parse_args()
    from esrecsys_amd import _lib
    from ratings_bench import _corpus
    assert torch.cuda.is_available(), "als_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    user, item, rating = _corpus(rng, 30000, 20000, 14, 1.1, 20.0)              # the ratings benchmark's corpus
    small = (torch.from_numpy(user).to(dev), torch.from_numpy(item).to(dev), torch.from_numpy(rating).to(dev))
    small_t = torch.rand(user.size, generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    configs, context = [], []
    for rank in (32, 64):
        configs.append(bench_config("ratings_bench", *small, rank, args, dev, lib, not args.skip_torch))
    context.append(quality("ratings_bench", *small, small_t, 32, args.quality_sweeps, dev))
    if not args.skip_large:
        large = device_corpus(140000, 27000, 156, 1.1, 20.0, dev, seed=2)
        for rank in (32, 64):
            configs.append(bench_config("synthetic_20M", *large[:3], rank, args, dev, lib, not args.skip_torch))
        context.append(quality("synthetic_20M", *large, 32, args.quality_sweeps, dev))
    print(json.dumps({"bench": "als", "device": torch.cuda.get_device_name(0), "reg": 0.1, "weighted_reg": True,
                      "reps": args.reps, "calls_per_window": args.inner, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
                      "f32_matrix_peak_flops": F32_MATRIX_FLOPS, "configs": configs, "leave_last_out": context}))


if __name__ == "__main__":
    main()

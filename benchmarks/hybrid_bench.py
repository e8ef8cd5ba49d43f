"""Hybrid BPR on one MI355X: the training step of ``factorization.HybridBPR`` at rank 64 and B = 65 536 on the Dice
benchmark's corpus shape (1 M documents of about 20 ids over 200 k items, split by ``split_holdout``; user = kept document)
with synthetic item features.  Every item has a latent cluster that also shapes the documents: a document draws most of its
ids from one cluster.  An item's features are its cluster id plus a few tags, most of them drawn from its cluster's own tag
pool and the rest from anywhere (noise).

Reported, as JSON lines (and written to ``profiles/hybrid/hybrid_bench.jsonl``):
  step       ms per step of ``train_steps`` and of every phase by HIP events; each bag kernel against the time its own
             bytes (feature rows read, feat and weight words, rows written) take at the 8 TB/s HBM peak;
  torch      the same step in plain torch (``embedding_bag`` with ``per_sample_weights`` for the composition, autograd's
             dense gradient, ``index_add_``-style Adagrad on the touched rows) in the same session;
  identity   the identity-only HybridBPR step against BPR's step on the same corpus: the price of the generality;
  quality    hold-out recall / nDCG at 10 / 100 / 500 against BPR trained as long; and the same metrics restricted to a tenth
             of the items, withheld from training and composed from their features only, against chance.
No target is fixed for any of these.

    python benchmarks/hybrid_bench.py [--reps 3] [--steps 32] [--train_steps 1500] [--skip_torch] [--skip_quality]
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

OUT = os.path.join(ROOT, "profiles", "hybrid")


def emit(rec, sink):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.append(line)


def clustered_corpus(rng, ndocs, V, clusters, mean, own_share):
    """(indices int32, offsets int64, cluster_of int64[V]): Poisson(mean) ids per document; a document picks a cluster and
    draws `own_share` of its ids from that cluster's items (Zipf inside the cluster), the rest from all items (Zipf)."""
    cluster_of = rng.integers(0, clusters, V)
    order = np.argsort(cluster_of, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.bincount(cluster_of, minlength=clusters))])
    n = np.maximum(rng.poisson(mean, ndocs), 2)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    total = int(off[-1])
    doc_cluster = np.repeat(rng.integers(0, clusters, ndocs), n)
    size = (starts[1:] - starts[:-1])[doc_cluster]
    inside = order[starts[doc_cluster] + (rng.zipf(1.2, total) - 1) % np.maximum(size, 1)]
    anywhere = (rng.zipf(1.2, total) - 1) % V
    indices = np.where(rng.random(total) < own_share, inside, anywhere).astype(np.int32)
    return indices, off, cluster_of


def item_features(rng, cluster_of, clusters, tags_per_item, pool, noise):
    """COO (item, feature): feature c for the item's cluster c, and tags_per_item tags (ids from `clusters` up): each from
    the cluster's own pool of `pool` tags, or from any pool with probability `noise`."""
    V = cluster_of.size
    item = np.repeat(np.arange(V), tags_per_item)
    own = np.repeat(cluster_of, tags_per_item)
    src = np.where(rng.random(item.size) < noise, rng.integers(0, clusters, item.size), own)
    tag = clusters + src * pool + rng.integers(0, pool, item.size)
    key = np.unique(np.concatenate([np.arange(V) * (1 << 32) + cluster_of, item * (1 << 32) + tag]))
    return key >> 32, key & 0xFFFFFFFF


def phase_times(model, K):
    """ms per step of the phases of K hybrid steps, by HIP events on the stream (the steps really train)."""
    from esrecsys_amd import ops
    ev = lambda: torch.cuda.Event(enable_timing=True)                        # noqa: E731
    dev, B = model.device, model.batch
    s0, s1, s2 = ev(), ev(), ev()
    s0.record()
    u, i, j, valid, _ = model.sample(K)
    s1.record()
    ij, valid2 = torch.cat([i, j], dim=1), torch.cat([valid, valid], dim=1)
    oo_u = torch.zeros((K, B + 1), dtype=torch.int64, device=dev)
    oo_i = torch.zeros((K, 2 * B + 1), dtype=torch.int64, device=dev)
    oo_u[:, 1:] = torch.cumsum(model._user_bags.lengths[u.to(torch.int64)], 1)
    oo_i[:, 1:] = torch.cumsum(model._item_bags.lengths[ij.to(torch.int64)], 1)
    sizes = torch.stack([oo_u[:, -1], oo_i[:, -1]]).cpu().numpy()
    s2.record()
    ar = torch.arange(2 * B, dtype=torch.int32, device=dev)
    ue, ie, ub, ib = model.user_embeddings, model.item_embeddings, model._user_bags, model._item_bags
    nfu, nfi = ue.shape[0], ie.shape[0]
    marks = [[ev() for _ in range(6)] for _ in range(K)]
    for k in range(K):
        m, Mu, Mi = marks[k], int(sizes[0, k]), int(sizes[1, k])
        m[0].record()
        P = ops.bag_sum(ue, *ub.args(), rows=u[k], failed=model._failed)
        Q = ops.bag_sum(ie, *ib.args(), rows=ij[k], failed=model._failed)
        m[1].record()
        _, _, grads = ops.bpr_fwd_bwd(P, Q, ar[:B], ar[:B], ar[B:], valid[k], 0.0, failed=model._failed)
        m[2].record()
        out_feat = torch.empty(Mu + Mi, dtype=torch.int32, device=dev)
        out_grads = torch.empty((Mu + Mi, model.rank), dtype=torch.float32, device=dev)
        ops.bag_expand(ue, *ub.args(), u[k], grads[:B], valid[k], oo_u[k], Mu, model.reg, out=(out_feat[:Mu], out_grads[:Mu]),
                       failed=model._failed)
        ops.bag_expand(ie, *ib.args(), ij[k], grads[B:], valid2[k], oo_i[k], Mi, model.reg,
                       out=(out_feat[Mu:], out_grads[Mu:]), failed=model._failed)
        m[3].record()
        s, p = ops.segment_sort_multi([out_feat[:Mu], out_feat[Mu:]], [0, nfu], nfu + nfi)
        m[4].record()
        ops.sparse_adagrad_multi([ue, ie], [model.user_accum, model.item_accum], [0, nfu, nfu + nfi], s, p, out_grads, model.lr)
        m[5].record()
    torch.cuda.synchronize()
    model.step += K
    model._composed = None
    med = lambda a, b: float(np.median([m[a].elapsed_time(m[b]) for m in marks]))   # noqa: E731
    occ = float((sizes[0] + sizes[1]).mean())
    return ({"sample_ms": s0.elapsed_time(s1) / K, "offsets_ms": s1.elapsed_time(s2) / K, "bag_sum_ms": med(0, 1),
             "fwd_bwd_ms": med(1, 2), "bag_expand_ms": med(2, 3), "sort_ms": med(3, 4), "update_ms": med(4, 5)}, occ)


def torch_step(ue, ie, ua, ia, ubag, ibag, u, ij, valid, reg, lr, eps=1e-7):
    """One hybrid step in plain torch on given triples: embedding_bag composes, autograd hands the gradient back (dense
    over the tables), Adagrad on the touched rows."""
    B = u.numel()
    tables = [ue.detach().requires_grad_(True), ie.detach().requires_grad_(True)]
    rows = []
    for table, (off, feat, w, lens), sel in ((tables[0], ubag, u), (tables[1], ibag, ij)):
        n = lens[sel]
        starts = torch.cumsum(n, 0) - n
        idx = torch.repeat_interleave(off[sel] - starts, n) + torch.arange(int(n.sum()), device=n.device)
        rows.append(torch.nn.functional.embedding_bag(feat[idx], table, starts, mode="sum",
                                                      per_sample_weights=None if w is None else w[idx]))
        # the L2 term over every occurrence of the valid triples' bags
        keep = torch.repeat_interleave((valid if sel is u else torch.cat([valid, valid])).to(torch.float32), n)
        rows.append(0.5 * reg * (keep[:, None] * table[feat[idx]] ** 2).sum())
    P, l2u, Q, l2i = rows
    d = (P * (Q[:B] - Q[B:])).sum(1)
    loss = -(torch.nn.functional.logsigmoid(d) * valid.to(torch.float32)).sum()
    (loss + l2u + l2i).backward()
    with torch.no_grad():
        for table, acc, t in ((ue, ua, tables[0]), (ie, ia, tables[1])):
            G = t.grad
            touched = torch.nonzero(G.abs().sum(1) > 0).reshape(-1)
            g = G[touched]
            a = acc[touched] + g * g
            acc[touched] = a
            table[touched] -= lr * g * torch.rsqrt(a + eps)
    return loss.detach()


def metrics(model, nq, truth, t_off, extra=None, only=None):
    """recall / nDCG at 10, 100, 500 of the first nq users; `only` = item ids the truth and the lists are restricted to"""
    from esrecsys_amd import evaluate
    dev = model.device
    ids, _, lens = model.recommend(torch.arange(nq, device=dev), k=500, extra_items=extra) if extra is not None else \
        model.recommend(torch.arange(nq, device=dev), k=500)
    q_truth, q_off = truth[:int(t_off[nq])], t_off[:nq + 1]
    m = evaluate.ranking_metrics(ids, lens, q_truth, q_off, ks=(10, 100, 500)).mean()
    return {"recall": [float(x) for x in m["recall"]], "ndcg": [float(x) for x in m["ndcg"]], "n_valid": int(m["n_valid"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32, help="steps per timed window")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--clusters", type=int, default=512)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--train_steps", type=int, default=1500)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--skip_torch", action="store_true")
    ap.add_argument("--skip_quality", action="store_true")
    args = ap.parse_args()
    from esrecsys_amd import evaluate, ops
    from esrecsys_amd import factorization as fz
    assert torch.cuda.is_available(), "hybrid_bench measures on an MI355X: no GPU, no number"
    dev = torch.device("cuda", 0)
    sink = []
    emit({"bench": "hybrid", "stage": "setup", "device": torch.cuda.get_device_name(0), "reps": args.reps,
          "steps_per_window": args.steps, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "geometry": ops.bag_geometry()}, sink)
    rng = np.random.default_rng(0)
    indices, off, cluster_of = clustered_corpus(rng, args.docs, args.vocab, args.clusters, 20, 0.7)
    f_item, f_id = item_features(rng, cluster_of, args.clusters, 3, 16, 0.25)
    ctx, c_off, truth, t_off, kept = evaluate.split_holdout(torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev))
    ctx_h, off_h = ctx.cpu().numpy().astype(np.int64), c_off.cpu().numpy().astype(np.int64)
    docs = np.repeat(np.arange(off_h.size - 1, dtype=np.int64), np.diff(off_h))

    def features_of(items):
        keep = np.isin(f_item, items)
        return f_item[keep], f_id[keep], None

    def hybrid(user, item, **kw):
        return fz.HybridBPR(user, item, item_features=features_of(np.unique(item)), rank=args.rank, batch=args.batch,
                            device=dev, **kw)

    t0 = time.perf_counter()
    model = hybrid(docs, ctx_h)
    torch.cuda.synchronize()
    D, B = model.rank, model.batch
    rec = {"bench": "hybrid", "stage": "step", "rank": D, "batch": B, "pairs": model.nnz, "users": int(model.users.numel()),
           "items": int(model.items.numel()), "item_feature_rows": int(model.item_embeddings.shape[0]),
           "item_bag_mean_length": float(model._item_bags.lengths.to(torch.float64).mean()),
           "build_seconds": round(time.perf_counter() - t0, 2)}
    model.train_steps(4)
    wall = min(_windows(lambda: model.train_steps(args.steps), args.reps, 1)) / args.steps
    phases, occ = phase_times(model, args.steps)
    # bytes of the two kernels per step: every occurrence reads a D-row, 4 bytes of feat (no weights here); sum writes 3 B
    # rows and reads 3 B row numbers and bag bounds; expand reads 3 B gradient rows and writes a D-row and 4 bytes per
    # occurrence
    sum_bytes = occ * (4 * D + 4) + 3 * B * (4 * D + 4 + 16)
    exp_bytes = occ * (4 * D + 4 + 4 * D + 4) + 3 * B * (4 * D + 4 + 16 + 4)
    rec.update({"train_steps_ms_per_step": round(wall * 1e3, 4), "triples_per_s": round(B / wall),
                **{k: round(v, 4) for k, v in phases.items()}, "phases_sum_ms": round(sum(phases.values()), 4),
                "occurrences_per_step": occ, "bag_sum_bytes": sum_bytes, "bag_expand_bytes": exp_bytes,
                "bag_sum_fraction_of_hbm_peak": round(sum_bytes / (phases["bag_sum_ms"] * 1e-3) / HBM_BYTES_PER_S, 4),
                "bag_expand_fraction_of_hbm_peak": round(exp_bytes / (phases["bag_expand_ms"] * 1e-3) / HBM_BYTES_PER_S, 4)})
    emit(rec, sink)

    if not args.skip_torch:
        K = 8
        u, i, j, valid, _ = model.sample(K)
        u64, ij64 = u.to(torch.int64), torch.cat([i, j], dim=1).to(torch.int64)
        bags = [(b.offsets, b.feat.to(torch.int64), b.weight, b.lengths) for b in (model._user_bags, model._item_bags)]
        ue, ie = model.user_embeddings.clone(), model.item_embeddings.clone()
        ua, ia = model.user_accum.clone(), model.item_accum.clone()
        state = {"k": 0}

        def one():
            k = state["k"] % K
            state["k"] += 1
            torch_step(ue, ie, ua, ia, bags[0], bags[1], u64[k], ij64[k], valid[k], model.reg, model.lr)
        one()
        t_torch = min(_windows(one, args.reps, K))
        t_ours = (sum(phases.values()) - phases["sample_ms"]) * 1e-3
        emit({"bench": "hybrid", "stage": "torch_restatement", "rank": D, "batch": B, "torch_ms_per_step": round(t_torch * 1e3, 4),
              "kernels_ms_per_step_without_sampler": round(t_ours * 1e3, 4), "torch_over_kernels": round(t_torch / t_ours, 2)},
             sink)
        del ue, ie, ua, ia
        torch.cuda.empty_cache()

    # the price of the generality: identity-only bags against BPR on the same pairs
    del model
    torch.cuda.empty_cache()
    plain = fz.HybridBPR(docs, ctx_h, rank=args.rank, batch=args.batch, device=dev)
    bpr = fz.BPR(docs, ctx_h, rank=args.rank, batch=args.batch, device=dev)
    plain.train_steps(4), bpr.train_steps(4)
    t_h = min(_windows(lambda: plain.train_steps(args.steps), args.reps, 1)) / args.steps
    t_b = min(_windows(lambda: bpr.train_steps(args.steps), args.reps, 1)) / args.steps
    emit({"bench": "hybrid", "stage": "identity_only_against_bpr", "hybrid_ms_per_step": round(t_h * 1e3, 4),
          "bpr_ms_per_step": round(t_b * 1e3, 4), "hybrid_over_bpr": round(t_h / t_b, 2)}, sink)
    del plain, bpr
    torch.cuda.empty_cache()

    if not args.skip_quality:
        nq = min(args.queries, int(kept.numel()))
        out = {"bench": "hybrid", "stage": "hold_out", "train_steps": args.train_steps, "queries": nq}
        for name, make in (("hybrid", lambda: hybrid(docs, ctx_h)),
                           ("bpr", lambda: fz.BPR(docs, ctx_h, rank=args.rank, batch=args.batch, device=dev))):
            t0 = time.perf_counter()
            m = make()
            losses = m.fit(args.train_steps)
            out[name] = dict(metrics(m, nq, truth, t_off), loss_last=float(np.mean(losses[-10:])), auc=m.auc(),
                             seconds=round(time.perf_counter() - t0, 2))
            del m
            torch.cuda.empty_cache()
        emit(out, sink)
        # cold start: a tenth of the items is withheld from the pairs and composed from features only; the truth and the
        # metric are restricted to those items
        items = np.unique(ctx_h)
        cold = items[np.random.default_rng(1).random(items.size) < 0.1]
        warm_pair = ~np.isin(ctx_h, cold)
        m = hybrid(docs[warm_pair], ctx_h[warm_pair])
        m.fit(args.train_steps)
        known = np.isin(f_id, m.item_feature_ids.cpu().numpy())             # (a tag only cold items carry was never seen)
        keep = np.isin(f_item, cold) & known
        extra = m.compose_items(f_item[keep], f_id[keep])
        truth_h, toff_h = truth.cpu().numpy().astype(np.int64), t_off.cpu().numpy().astype(np.int64)
        tdoc = np.repeat(np.arange(toff_h.size - 1), np.diff(toff_h))
        tk = np.isin(truth_h, extra[0].cpu().numpy())
        cold_truth = torch.from_numpy(truth_h[tk].astype(np.int32)).to(dev)
        cold_off = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(tdoc[tk], minlength=toff_h.size - 1))])).to(dev)
        users_known = m._positions(torch.arange(nq, device=dev), m.users) >= 0
        # rank the cold items alone: the known items are dropped from the lists by scoring the extra items only
        cand_ids, cand_rows = extra
        X = m.user_rows()
        upos = m._positions(torch.arange(nq, device=dev), m.users).to(torch.int64).clamp(min=0)
        _, top = ops.retrieve_topk(X[upos].contiguous(), cand_rows, 500, mode="exact")
        rec_ids = cand_ids[top.to(torch.int64)].to(torch.int32).contiguous()
        lens = torch.where(users_known, torch.full((nq,), 500, dtype=torch.int32, device=dev),
                           torch.zeros(nq, dtype=torch.int32, device=dev))
        mm = evaluate.ranking_metrics(rec_ids, lens, cold_truth[:int(cold_off[nq])], cold_off[:nq + 1], ks=(10, 100, 500)).mean()
        emit({"bench": "hybrid", "stage": "cold_start", "cold_items": int(cand_ids.numel()),
              "cold_truth_entries": int(cold_off[nq]), "recall": [float(x) for x in mm["recall"]],
              "ndcg": [float(x) for x in mm["ndcg"]], "n_valid": int(mm["n_valid"]),
              "chance_recall": [k / max(int(cand_ids.numel()), 1) for k in (10, 100, 500)]}, sink)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "hybrid_bench.jsonl"), "w") as f:
        f.write("\n".join(sink) + "\n")


if __name__ == "__main__":
    main()

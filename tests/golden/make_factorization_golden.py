"""Generates tests/golden/factorization_parent.json (run from the repo root on an MI355X:
``python tests/golden/make_factorization_golden.py [--out FILE] [--families fpmc,sgns]``; with ``--families`` only those
are trained and the other entries of the committed file are carried over unchanged).

The models of esrecsys_amd/factorization.py are functions of their inputs and the seed, so the fixture holds no
numbers, only SHA-256 digests: per small model, of every factor / embedding / accumulator table, of the returned loss
lists (as float64 bytes) and of a few outputs (recommend, auc, fold_in).  It was written once, at the commit BEFORE the
models were given one base class, and pins that the rewrite trains bit for bit what its parent trained: the same
generator draws, the same ops calls in the same order.  The families ``fpmc`` and ``sgns`` were appended at the commit
BEFORE the sampled-SGD models were given one sampler shell, one logistic and one trainer base, and pin that rewrite in the
same way.  tests/test_gpu_factorization_golden.py retrains the models through ``compute()`` below and compares.

Data: a seeded NumPy generator, 40 users over 1300 items.  User 0 has about 1100 items (longer than a workgroup's
``chunk * chunks_per_workgroup`` of ``ops.als_geometry()``), users 1-4 have 300 to 900 (more than one chunk) and the rest are
short (one wave).  The constructors index through ``torch.unique``, so no training row is empty; the empty row goes through
the row solve as an ``ImplicitALS.fold_in`` document without a known id."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "factorization_parent.json")
NU, NI = 40, 1300


def digest(value):
    """SHA-256 of a tensor's / array's bytes behind its dtype and shape; a list of python floats goes in as float64."""
    import torch
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    elif isinstance(value, (list, tuple, float)):
        value = np.asarray(value, np.float64)
    value = np.ascontiguousarray(value)
    h = hashlib.sha256(("%s%s" % (value.dtype.str, value.shape)).encode())
    h.update(value.tobytes())
    return h.hexdigest()


def pairs():
    """(user, item) int64, every pair once, in a shuffled order: the row lengths of the module text."""
    rng = np.random.default_rng(20240)
    lengths = np.concatenate([[1100, 300, 500, 700, 900], rng.integers(1, 60, NU - 5)])
    user = np.repeat(np.arange(NU, dtype=np.int64) * 3 + 2, lengths)             # ids that are not positions
    item = np.concatenate([rng.choice(NI, int(n), replace=False) for n in lengths]).astype(np.int64) * 2 + 5
    order = rng.permutation(user.size)
    return user[order], item[order], rng


def _queries(user):
    """Users 1 and 5 to 16 (user 0's seen items alone exceed what recommend can exclude) and id 1, which is no user."""
    return np.concatenate([np.unique(user)[[1] + list(range(5, 17))], [1]])


def als_models(out):
    import torch
    from esrecsys_amd import factorization as fz
    user, item, rng = pairs()
    rating = rng.integers(1, 6, user.size).astype(np.float32)
    strength = rng.uniform(0.5, 3.0, user.size)
    # implicit feedback: some events repeat (their strengths add)
    again = rng.integers(0, user.size, 200)
    iu, ii, istr = np.concatenate([user, user[again]]), np.concatenate([item, item[again]]), \
        np.concatenate([strength, rng.uniform(0.5, 3.0, 200)])
    new_docs = np.concatenate([np.unique(item)[:30], [4], np.unique(item)[100:160]])     # (id 4 is no item)
    new_off = np.array([0, 30, 31, 31, 91], np.int64)                            # document 1: no known id, 2: empty
    for rank, weighted in ((8, True), (40, False)):
        for per_launch in (None, 7):
            m = fz.RatingsALS(user, item, rating, rank=rank, reg=0.1, weighted_reg=weighted, center="user", seed=3,
                              max_rows_per_launch=per_launch)
            history = m.fit(sweeps=2)
            rec = m.recommend(_queries(user), k=20)
            out["RatingsALS rank=%d weighted_reg=%s max_rows_per_launch=%s" % (rank, weighted, per_launch)] = [
                ("user_factors", digest(m.user_factors)), ("item_factors", digest(m.item_factors)),
                ("user_mean", digest(m.user_mean)), ("history", digest(history)), ("residuals", digest(m.residuals())),
                ("recommend ids", digest(rec[0])), ("recommend scores", digest(rec[1])), ("recommend lengths", digest(rec[2]))]
            m = fz.ImplicitALS(iu, ii, istr, rank=rank, reg=0.05, alpha=10.0, weighted_reg=not weighted, seed=4,
                               max_rows_per_launch=per_launch)
            history = m.fit(sweeps=2)
            rec = m.recommend(_queries(user), k=20)
            folded = m.fold_in(new_docs, new_off)
            assert not bool(folded[1:3].any())
            docs = m.recommend_documents(new_docs, new_off, k=10)
            out["ImplicitALS rank=%d weighted_reg=%s max_rows_per_launch=%s" % (rank, not weighted, per_launch)] = [
                ("user_factors", digest(m.user_factors)), ("item_factors", digest(m.item_factors)),
                ("history", digest(history)), ("score", digest(m.score(user[:50], item[:50]))),
                ("recommend ids", digest(rec[0])), ("recommend scores", digest(rec[1])), ("recommend lengths", digest(rec[2])),
                ("fold_in", digest(folded)), ("recommend_documents ids", digest(docs[0])),
                ("recommend_documents scores", digest(docs[1]))]
    torch.cuda.synchronize()


def _triple_tables(m, losses):
    return [("user_factors", digest(m.user_factors)), ("item_factors", digest(m.item_factors)),
            ("user_accum", digest(m.user_accum)), ("item_accum", digest(m.item_accum)), ("losses", digest(losses)),
            ("step", digest(float(m.step))), ("auc", digest(m.auc()))]


def bpr_models(out):
    from esrecsys_amd import factorization as fz
    user, item, _ = pairs()
    for rank in (4, 20, 64, 128):
        for optimizer in fz.OPTIMIZERS:
            m = fz.BPR(user, item, rank=rank, reg=0.02, lr=0.05, optimizer=optimizer, batch=300, seed=5)
            losses = m.train_steps(3) + m.train_steps(2)
            out["BPR rank=%d optimizer=%s" % (rank, optimizer)] = _triple_tables(m, losses)
            if rank <= fz.max_rank():                                            # (recommend re-scores by the ALS predict kernel)
                rec = m.recommend(_queries(user), k=20)
                out["BPR rank=%d optimizer=%s" % (rank, optimizer)] += [
                    ("recommend ids", digest(rec[0])), ("recommend scores", digest(rec[1])),
                    ("recommend lengths", digest(rec[2]))]


def warp_models(out):
    from esrecsys_amd import factorization as fz
    user, item, _ = pairs()
    for rank_weight in fz.RANK_WEIGHTS:
        # (init_scale 1 and a small margin: scores of order sqrt(rank), so most candidates keep the margin and a search
        # walks several of its max_trials, as many as the factors decide)
        m = fz.WARP(user, item, rank=20, reg=0.02, lr=0.05, batch=300, seed=6, init_scale=1.0, max_trials=8, margin=0.1,
                    rank_weight=rank_weight)
        triples = m.step_triples()
        losses = m.train_steps(3)
        out["WARP rank=20 max_trials=8 rank_weight=%s" % rank_weight] = _triple_tables(m, losses) + [
            ("mean_trials", digest(m.mean_trials)), ("step_triples", digest(np.stack([t.cpu().numpy() for t in triples])))]


def hybrid_models(out):
    from esrecsys_amd import factorization as fz
    user, item, rng = pairs()
    items, users = np.unique(item), np.unique(user)
    n_tags = rng.integers(1, 4, items.size)
    f_item = np.repeat(items, n_tags)
    f_tag = np.concatenate([rng.choice(50, int(n), replace=False) for n in n_tags]).astype(np.int64) + 7
    f_weight = rng.uniform(0.25, 2.0, f_item.size).astype(np.float32)
    n_groups = rng.integers(1, 3, users.size)
    g_user = np.repeat(users, n_groups)
    g_group = np.concatenate([rng.choice(6, int(n), replace=False) for n in n_groups]).astype(np.int64)
    new_item = np.repeat(np.array([4001, 4003, 4000], np.int64), [2, 1, 3])
    new_tag = np.array([7, 9, 30, 8, 10, 56], np.int64)
    assert np.isin(new_tag, f_tag).all()                                         # only tags the model saw
    new_weight = np.array([1.0, 0.5, 2.0, 1.5, 0.75, 1.25], np.float32)
    for identity in ((True, True), (False, True)):
        m = fz.HybridBPR(user, item, user_features=(g_user, g_group, None), item_features=(f_item, f_tag, f_weight),
                         identity=identity, rank=20, reg=0.02, lr=0.05, batch=300, seed=7)
        losses = m.train_steps(3)
        extra = m.compose_items(new_item, new_tag, new_weight)
        rec = m.recommend(_queries(user), k=20, extra_items=extra)
        out["HybridBPR rank=20 identity=%s" % (identity,)] = [
            ("user_embeddings", digest(m.user_embeddings)), ("item_embeddings", digest(m.item_embeddings)),
            ("user_accum", digest(m.user_accum)), ("item_accum", digest(m.item_accum)), ("losses", digest(losses)),
            ("user_factors", digest(m.user_factors)), ("item_factors", digest(m.item_factors)), ("auc", digest(m.auc())),
            ("compose_items ids", digest(extra[0])), ("compose_items rows", digest(extra[1])),
            ("recommend ids", digest(rec[0])), ("recommend scores", digest(rec[1])), ("recommend lengths", digest(rec[2]))]


def _sequences(item):
    """Given sequences over the known items: five ids, an empty one, one with an id that is no item (4), one unknown id
    alone and a long one (more than any window); as (indices, doc_offsets)."""
    items = np.unique(item)
    docs = [items[:5], items[:0], np.concatenate([items[10:12], [4], items[40:41]]), np.array([4], np.int64), items[100:130]]
    return np.concatenate(docs).astype(np.int64), np.concatenate([[0], np.cumsum([d.size for d in docs])]).astype(np.int64)


def fpmc_models(out):
    """``pairs()`` read as sequences (the shuffled order is the order of events, or `time` with ties decides)."""
    from esrecsys_amd import factorization as fz
    user, item, rng = pairs()
    time = rng.integers(0, 50, user.size)
    seq, seq_off = _sequences(item)
    seq_users = np.array([np.unique(user)[1], 1, np.unique(user)[7], np.unique(user)[8], 1], np.int64)    # (1 is no user)
    for rank, window, optimizer, timed in ((4, 1, "adagrad", False), (20, 3, "adagrad", True), (20, 3, "sgd", False),
                                           (64, 8, "adagrad", True), (128, 3, "adagrad", False)):
        m = fz.FPMC(user, item, time=time if timed else None, window=window, rank=rank, reg=0.02, lr=0.05,
                    optimizer=optimizer, batch=300, seed=8)
        losses = m.train_steps(3) + m.train_steps(2)
        name = "FPMC rank=%d window=%d optimizer=%s time=%s" % (rank, window, optimizer, timed)
        out[name] = _triple_tables(m, losses) + [
            ("next_factors", digest(m.next_factors)), ("prev_factors", digest(m.prev_factors)),
            ("next_accum", digest(m.next_accum)), ("prev_accum", digest(m.prev_accum))]
        if rank <= fz.predict_max_rank() // 2:                                   # (serving re-scores rows of 2 rank)
            rec = m.recommend(_queries(user), k=20)
            by_seq = m.recommend_sequences(seq, seq_off, k=20, users=seq_users)
            session = m.recommend_sequences(seq, seq_off, k=20, exclude_seen=False)
            out[name] += [("recommend ids", digest(rec[0])), ("recommend scores", digest(rec[1])),
                          ("recommend lengths", digest(rec[2]))]
            out[name] += [("recommend_sequences %s %s" % (how, what), digest(t)) for how, r in
                          (("users", by_seq), ("session", session)) for what, t in zip(("ids", "scores", "lengths"), r)]


def sgns_models(out):
    """``pairs()`` read as documents: the user is the document."""
    from esrecsys_amd import factorization as fz
    user, item, rng = pairs()
    time = rng.integers(0, 50, user.size)
    seq, seq_off = _sequences(item)
    similar_to = np.concatenate([np.unique(item)[[0, 3, 700, -1]], [4]])       # (id 4 is no item)
    for rank, negatives, window, optimizer, timed in ((4, 1, 1, "adagrad", False), (20, 5, 5, "adagrad", True),
                                                      (20, 5, 5, "sgd", False), (64, 16, 5, "adagrad", False),
                                                      (128, 5, 1, "adagrad", True)):
        m = fz.SGNS(user, item, time=time if timed else None, window=window, negatives=negatives, rank=rank, reg=0.02,
                    lr=0.05, optimizer=optimizer, batch=300, seed=9)
        losses = m.train_steps(3) + m.train_steps(2)
        sim = m.similar_items(similar_to, k=20)
        rec = m.recommend_sequences(seq, seq_off, k=20)
        out["SGNS rank=%d negatives=%d window=%d optimizer=%s time=%s" % (rank, negatives, window, optimizer, timed)] = [
            ("in_factors", digest(m.in_factors)), ("out_factors", digest(m.out_factors)),
            ("in_accum", digest(m.in_accum)), ("out_accum", digest(m.out_accum)), ("losses", digest(losses)),
            ("step", digest(float(m.step))), ("accuracy", digest(m.accuracy())),
            ("similar_items ids", digest(sim[0])), ("similar_items scores", digest(sim[1])),
            ("similar_items lengths", digest(sim[2])), ("recommend_sequences ids", digest(rec[0])),
            ("recommend_sequences scores", digest(rec[1])), ("recommend_sequences lengths", digest(rec[2]))]


FAMILIES = {"als": als_models, "bpr": bpr_models, "warp": warp_models, "hybrid": hybrid_models, "fpmc": fpmc_models,
            "sgns": sgns_models}


def compute(family):
    """{model name: [(what, sha256), ...] in a fixed order} of one family of FAMILIES, trained on the current device."""
    out = {}
    FAMILIES[family](out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    result = {}
    families = list(FAMILIES)
    if "--families" in sys.argv:                       # only these are trained; the file's other entries stay as they are
        families = sys.argv[sys.argv.index("--families") + 1].split(",")
        with open(OUT) as f:
            result = {k: [tuple(p) for p in v] for k, v in json.load(f).items()}
    for name in families:
        result.update(compute(name))
    with open(path, "w") as f:
        json.dump({k: [list(p) for p in v] for k, v in result.items()}, f, indent=1)
        f.write("\n")
    print("wrote %d models to %s" % (len(result), path))

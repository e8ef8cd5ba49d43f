"""SHA-256 over every output of the three units that combine long runs, for batches with ONE hot id.

    python profiles/long_runs/digests.py TREE OUT.json

TREE is the root of a built checkout (its esrecsys_amd package and library are the ones used), so the same script runs
against the tree before a change and the tree after it; the two JSON files must then be equal.

A hot run of L occurrences whose head sits at sorted position h is cut into K + 1 partials (esr_segment.h).  L and h are
chosen so that K + 1 takes the values 2, NG - 1, NG, NG + 1, 4 NG - 1, 4 NG, 4 NG + 1 for every number of row groups per
workgroup NG the kernels run with at D = 128 and D = 6 (8, 16, 32), and 258 (more than 256 continuation chunks: the K
count's second pass), with the head at alignment 0 and CHUNK - 1 of the chunk (32; 8 for the stamped triplet step, which
31 also puts on its last position).  One uniform and one Zipf batch of 3000 ids per unit on top.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[1])
from esrecsys_amd import ops  # noqa: E402
from esrecsys_amd._lib import GLOVE_DIAGONAL, GLOVE_REFERENCE  # noqa: E402

dev = torch.device("cuda", 0)
out = {}
PARTIALS = sorted({2, 258} | {m * ng + d for ng in (8, 16, 32) for m in (1, 4) for d in (-1, 0, 1)})
ALIGN = (0, 31)
WIDTHS = (128, 6)
TRIP_ENV = ("ESR_TRIPLET_STEP", "ESR_TRIPLET_DIRECT_LANES", "ESR_BF16_VEC8")
TRIP_MODES = {"direct": {}, "few": {"ESR_TRIPLET_DIRECT_LANES": "few"}, "stamped": {"ESR_TRIPLET_STEP": "stamped"},
              "vec8": {"ESR_BF16_VEC8": "1"}}


def put(name, *tensors):
    for i, t in enumerate(tensors):
        t = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
        out["%s/%d" % (name, i)] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run_length(partials, align, chunk):
    """the shortest run with its head at `align` inside a chunk that is cut into `partials` partial sums"""
    head_chunk = chunk + (chunk - align) % chunk
    return head_chunk + (partials - 2) * chunk + 1


def hot_list(n, V, length, align, rng):
    """int32 [n], shuffled: id 1 `length` times, id 0 `align` times (what sorts in front of the hot run), other ids once"""
    assert n >= length + align and V >= n + 2
    rest = 2 + rng.permutation(V - 2)[:n - length - align]
    ids = np.concatenate([np.full(length, 1), np.zeros(align, np.int64), rest]).astype(np.int32)
    rng.shuffle(ids)
    return ids


def zipf(V, n, rng):
    w = 1.0 / np.arange(1, V + 1)
    return rng.permutation(V)[rng.choice(V, size=n, p=w / w.sum())].astype(np.int32)


def id_lists(n, V, chunk, rng):
    """(name, ids) of every batch of one unit: the ladder, then a uniform and a Zipf batch"""
    for p in PARTIALS:
        for a in ALIGN:
            length = run_length(p, a, chunk)
            ids = hot_list(max(n, length + a + 64), V, length, a, rng)
            # the run was parked and is cut as asked: head at sorted position a, p partial sums by the kernels' rule
            pos = np.flatnonzero(np.sort(ids) == 1)
            nxt = (int(pos[0]) + 2 * chunk - 1) // chunk * chunk
            assert int(pos[0]) == a and 1 - (-(int(pos[-1]) + 1 - nxt) // chunk) == p >= 2
            yield "hot/P%d/a%d" % (p, a), ids
    yield "uniform/n3000", rng.integers(0, V, 3000).astype(np.int32)
    yield "zipf/n3000", zipf(V, 3000, rng)


def dev_t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.to(dtype) if dtype is not None else t


def table(rng, V, D, dtype=torch.float32):
    return dev_t((rng.standard_normal((V, D)) * 0.3).astype(np.float32), dtype)


# ---- the segment engine: Adagrad over two fused tables, and plain SGD -------------------------------------------------
def segment(D):
    rng = np.random.default_rng([1, D])
    V = 12000
    for name, ids in id_lists(256, V, 32, rng):
        n = ids.size
        grads = dev_t((rng.standard_normal((n, D)) * 0.1).astype(np.float32))
        half = V // 2  # two fused tables of V / 2 rows: the ids are their virtual rows
        tabs, accs = [table(rng, half, D), table(rng, half, D)], [table(rng, half, D).abs(), table(rng, half, D).abs()]
        srt, prm = ops.segment_sort(dev_t(ids), V)
        ops.sparse_adagrad_multi(tabs, accs, [0, half, V], srt, prm, grads.clone(), 0.05)
        put("segment_adagrad_multi/D%d/%s" % (D, name), *tabs, *accs)
        one = table(rng, V, D)
        ops.sparse_sgd(one, srt, prm, grads.clone(), 0.05)
        put("segment_sgd/D%d/%s" % (D, name), one)


# ---- the GloVe one-pass step: both modes, f32 and bf16 rows -----------------------------------------------------------
def glove(D):
    rng = np.random.default_rng([2, D])
    V = 12000
    for name, ids in id_lists(256, V, 32, rng):
        n = ids.size + (ids.size & 1)
        flat = np.concatenate([ids, ids[:n - ids.size]])
        inputs = dev_t(flat.reshape(2, n // 2))
        target = dev_t(np.exp(rng.uniform(np.log(0.1), np.log(1000.0), n // 2)).astype(np.float32))
        emb0, acc0 = table(rng, V, D), table(rng, V, D).abs() + 0.1
        bias0 = dev_t((rng.standard_normal(V) * 0.05).astype(np.float32))
        for mode_name, mode in (("reference", GLOVE_REFERENCE), ("diagonal", GLOVE_DIAGONAL)):
            for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                emb, shadow = emb0.to(dt), torch.zeros_like(emb0, dtype=dt)
                loc = torch.zeros(V, dtype=torch.uint8, device=dev)
                acc, bias, bacc = acc0.clone(), bias0.clone(), torch.full((V,), 0.1, device=dev)
                loss = ops.glove_train_step(emb, shadow, loc, acc, bias, bacc, inputs, target, mode, 0.05, stamp=1)
                put("glove_%s_%s/D%d/%s" % (mode_name, dt_name, D, name), emb, shadow, loc, acc, bias, bacc, loss)


# ---- the triplet one-pass step: direct, few lanes, stamped, bf16 with 8-element chunks ---------------------------------
def triplet(D):
    V = 12000
    for mode, env in TRIP_MODES.items():
        for var in TRIP_ENV:
            os.environ.pop(var, None)
        os.environ.update(env)
        rng = np.random.default_rng([3, D])
        for name, sid in id_lists(256, V, 8 if mode == "stamped" else 32, rng):
            B = sid.size
            pid = hot_list(B, V, int((sid == 1).sum()), int((sid == 0).sum()), rng) if name.startswith("hot") else \
                rng.permutation(sid)
            nid = rng.integers(2, V, B).astype(np.int32)
            ids = [dev_t(x) for x in (sid, pid, nid)]
            for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                if (mode == "stamped" and dt_name == "bf16") or (mode == "vec8" and dt_name == "f32"):
                    continue  # stamped: f32 rows only; vec8: bf16 rows only
                rs = np.random.default_rng([4, D])
                s, p = table(rs, V, D, dt), table(rs, V, D, dt)
                sa, pa = table(rs, V, D).abs() + 0.1, table(rs, V, D).abs() + 0.1
                if mode == "stamped":
                    s1, p1 = torch.zeros_like(s), torch.zeros_like(p)
                    sl, pl = (torch.zeros(V, dtype=torch.uint8, device=dev) for _ in range(2))
                    loss = ops.triplet_train_step(s, s1, sl, sa, p, p1, pl, pa, *ids, 0.1, float(B), 0.05, stamp=1)
                    put("triplet_stamped_f32/D%d/%s" % (D, name), s, s1, sl, sa, p, p1, pl, pa, loss)
                else:
                    loss = ops.triplet_train_step(s, None, None, sa, p, None, None, pa, *ids, 0.1, float(B), 0.05)
                    put("triplet_%s_%s/D%d/%s" % (mode, dt_name, D, name), s, sa, p, pa, loss)
    for var in TRIP_ENV:
        os.environ.pop(var, None)


def grouped(digests):
    """one SHA-256 per case "<entry point>/<width>/<batch>" over the sorted (tensor, digest) lines of the case: a
    difference names the entry point, the width, the partial count and the alignment"""
    groups = {}
    for key in sorted(digests):
        g = groups.setdefault(key.rsplit("/", 1)[0], [hashlib.sha256(), 0])
        g[0].update(("%s=%s\n" % (key, digests[key])).encode())
        g[1] += 1
    return {name: "%s over %d tensors" % (h.hexdigest(), cnt) for name, (h, cnt) in groups.items()}


for D in WIDTHS:
    segment(D)
    glove(D)
    triplet(D)
torch.cuda.synchronize()
with open(sys.argv[2], "w") as f:
    json.dump(grouped(out), f, indent=0, sort_keys=True)
print("%d tensors in %d groups -> %s" % (len(out), len(grouped(out)), sys.argv[2]))

"""SHA-256 over every output of every entry point of the sort unit for a fixed, seeded list of shapes.

    python profiles/sort_host/digests.py TREE OUT.json

TREE is the root of a built checkout (its esrecsys_amd package and library are the ones used), so the same script
runs against the tree before a change and the tree after it; the two JSON files must then be equal.  The shapes put a
case on each side of every threshold of the sort unit's path plan (see NOTES.md).
"""
import hashlib
import json
import sys

import numpy as np
import torch

sys.path.insert(0, sys.argv[1])
from esrecsys_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
rng = np.random.default_rng(20240607)
out = {}


def put(name, *tensors):
    for i, t in enumerate(tensors):
        out["%s/%d" % (name, i)] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def grouped(digests):
    """one SHA-256 per "<entry point>/<size>" over the sorted (case, tensor digest) lines of the group: the files stay
    short, and a difference still names the entry point and the size class"""
    groups = {}
    for key in sorted(digests):
        g = groups.setdefault("/".join(key.split("/")[:2]), [hashlib.sha256(), 0])
        g[0].update(("%s=%s\n" % (key, digests[key])).encode())
        g[1] += 1
    return {name: "%s over %d tensors" % (h.hexdigest(), cnt) for name, (h, cnt) in groups.items()}


NB = 8
SORT_N = [512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 262144, 262145,
          1 << 21, (1 << 21) + 1]
SORT_V = [5000, 1 << 21, (1 << 21) + 1, (1 << 31) - 1]   # many equal ids; the last 32-bit composite; wide ids; three passes
raw = torch.from_numpy(rng.integers(0, (1 << 31) - 1, (NB, max(SORT_N)), dtype=np.int64).astype(np.int32)).to(dev)


def ids_of(b, n, V):
    return (raw[b, :n] % V).contiguous()


def segments(b, n, nseg, V):
    """the list of batch b as nseg segments whose virtual ids stay below V; nseg = 3 has an empty middle segment"""
    if nseg == 1:
        return [ids_of(b, n, V)], (0,)
    a, half = n // 3, V // 2
    x = raw[b, :n]
    return [(x[:a] % half).contiguous(), x[:0].contiguous(), (x[a:] % (V - half)).contiguous()], (0, half, half)


for n in SORT_N:
    for V in SORT_V:
        put("sort/n%d/V%d" % (n, V), *ops.segment_sort(ids_of(0, n, V), V))
        segs, offs = segments(1, n, 3, V)
        put("sort_multi/n%d/V%d" % (n, V), *ops.segment_sort_multi(segs, offs, V))
        for nb in (1, 2, 8):
            for nseg in (1, 3):
                lists = [segments(b, n, nseg, V) for b in range(nb)]
                put("sort_batched/n%d/V%d/nb%d/nseg%d" % (n, V, nb, nseg),
                    *ops.segment_sort_batched([s for s, _ in lists], lists[0][1], V))

BUCKET_N = [2048, 2049, 32768, 32769, 1 << 20, (1 << 20) + 1]
for n in BUCKET_N:
    for world in (1, 3, 8, 9):
        V = 1_000_003
        put("bucket/n%d/w%d" % (n, world), *ops.bucket_ids_by_owner(ids_of(0, n, V), world, want_inverse=True))
        segs, offs = segments(1, n, 3, V)
        put("bucket_multi/n%d/w%d" % (n, world), *ops.bucket_ids_by_owner(segs, world, want_inverse=True, offsets=offs))
        for nb in (1, 2, 8):
            for nseg in (1, 3):
                lists = [segments(b, n, nseg, V) for b in range(nb)]
                put("bucket_batched/n%d/w%d/nb%d/nseg%d" % (n, world, nb, nseg),
                    *ops.bucket_ids_by_owner_batched([s for s, _ in lists], world, lists[0][1]))

# scores rounded to a few values per column: equal keys test the stable order
for V in (1000, 4097, 40000):
    for T in (1, 8, 9):
        scores = torch.from_numpy(np.round(rng.standard_normal((V, T)) * 8).astype(np.float32) / 8).to(dev)
        put("argsort/V%d/T%d" % (V, T), ops.argsort_columns(scores))
cand = torch.from_numpy((rng.integers(-8, 9, (5000, 32)) / 4.0).astype(np.float32)).to(dev)
for nq in (1, 8, 9):
    q = torch.from_numpy((rng.integers(-8, 9, (nq, 32)) / 4.0).astype(np.float32)).to(dev)
    for k in (1024, 1025):
        put("topk/nq%d/k%d" % (nq, k), *ops.score_topk(q, cand, k))

torch.cuda.synchronize()
with open(sys.argv[2], "w") as f:
    json.dump(grouped(out), f, indent=0, sort_keys=True)
print("%d tensors in %d groups -> %s" % (len(out), len(grouped(out)), sys.argv[2]))

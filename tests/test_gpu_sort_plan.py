"""GPU: the sort unit's size functions and its dispatchers agree, and what the id-list builders put into unused
segment slots does not matter.

Every entry point of esr_sort.hip that takes a workspace is called through the C ABI with exactly the bytes its
*_workspace_bytes function states -- it must give the stable order -- and with one byte less -- it must return
ESR_EWORKSPACE under its own name.  The list lengths are the smallest of each path that uses a workspace: 2049 (tile
sort + rank), 4097 wide ids (radix, where the 64-bit one-workgroup sort ends), 32769 (radix), 2^21 + 1 (the
column-scanned radix form); the bucket's radix path (world 9: more owners than the counting kernels take) at 2049 and
32769."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EWORKSPACE = -3
WIDE = (1 << 21) + 1      # ids that no longer fit the 32-bit (id << 11 | position) composite
SORT_CASES = [(2049, 100_000), (4097, WIDE), (32769, 100_000), ((1 << 21) + 1, 100_000)]
BUCKET_CASES = [(2049, 9), (32769, 9)]

_ids_cache = {}


def ids_for(dev, nlists, n, V):
    """[nlists, n] int32 ids below V (seeded), on the host and on the device: made once per shape, never written"""
    key = (nlists, n, V)
    if key not in _ids_cache:
        h = np.random.default_rng(n + V).integers(0, V, (nlists, n)).astype(np.int32)
        _ids_cache[key] = (h, torch.from_numpy(h).to(dev))
    return _ids_cache[key]


def stable_sort(h):
    perm = np.argsort(h, kind="stable").astype(np.int32)
    return h[perm], perm


def stable_bucket(h, world):
    perm = np.argsort(h % world, kind="stable").astype(np.int32)
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(h.size, dtype=np.int32)
    return h[perm] // world, perm, np.bincount(h % world, minlength=world).astype(np.int64), inverse


def segs_of(row, cuts):
    """the device row split at `cuts` into its segments (empty pieces included)"""
    edges = [0] + list(cuts) + [row.numel()]
    return [row[a:b] for a, b in zip(edges[:-1], edges[1:])]


def triple(lists):
    from esrecsys_amd import ops
    return (ops.ptr_array([t for segs in lists for t in segs]), ops.i64_array([t.numel() for t in lists[0]]),
            ops.i64_array([0] * len(lists[0])))


def sort_calls(dev, n, V):
    """name -> (bytes needed, call(ws, ws_bytes) -> (rc, sorted, perm), host ids [lists, n])"""
    from esrecsys_amd import _lib, ops
    lib = _lib.load()
    h, d = ids_for(dev, 2, n, V)
    out = {}

    def outputs(nl):
        return torch.empty((nl, n), dtype=torch.int32, device=dev), torch.empty((nl, n), dtype=torch.int32, device=dev)

    def single(ws, nbytes):
        s, p = outputs(1)
        return lib.esr_segment_sort_ids(d[0].data_ptr(), n, V, s.data_ptr(), p.data_ptr(), ws.data_ptr(), nbytes,
                                        ops._stream()), s, p
    out["esr_segment_sort_ids"] = (lib.esr_segment_sort_workspace_bytes(n), single, h[:1])

    def multi(ws, nbytes):
        s, p = outputs(1)
        ptrs, cnt, off = triple([segs_of(d[0], (n // 3,))])
        return lib.esr_segment_sort_ids_multi(ptrs, cnt, off, 2, V, s.data_ptr(), p.data_ptr(), ws.data_ptr(), nbytes,
                                              ops._stream()), s, p
    out["esr_segment_sort_ids_multi"] = (lib.esr_segment_sort_workspace_bytes(n), multi, h[:1])

    for nb in (1, 2):
        def batched(ws, nbytes, nb=nb):
            s, p = outputs(nb)
            ptrs, cnt, off = triple([segs_of(d[b], (n // 3,)) for b in range(nb)])
            return lib.esr_segment_sort_ids_batched(ptrs, cnt, off, 2, nb, V, s.data_ptr(), p.data_ptr(), ws.data_ptr(),
                                                    nbytes, ops._stream()), s, p
        out["esr_segment_sort_ids_batched/%d" % nb] = (lib.esr_segment_sort_batched_workspace_bytes(n, nb), batched, h[:nb])
    return out


def bucket_calls(dev, n, world):
    """name -> (bytes needed, call(ws, ws_bytes) -> (rc, local_rows, perm, counts, inverse), host ids [lists, n])"""
    from esrecsys_amd import _lib, ops
    lib = _lib.load()
    h, d = ids_for(dev, 2, n, 1_000_003)
    out = {}

    def outputs(nl):
        return (torch.empty((nl, n), dtype=torch.int32, device=dev), torch.empty((nl, n), dtype=torch.int32, device=dev),
                torch.empty((nl, world), dtype=torch.int64, device=dev), torch.empty((nl, n), dtype=torch.int32, device=dev))

    def single(ws, nbytes):
        lr, p, c, inv = outputs(1)
        return lib.esr_bucket_ids_by_owner(d[0].data_ptr(), n, world, lr.data_ptr(), p.data_ptr(), inv.data_ptr(),
                                           c.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), lr, p, c, inv
    out["esr_bucket_ids_by_owner"] = (lib.esr_bucket_workspace_bytes(n), single, h[:1])

    def multi(ws, nbytes):
        lr, p, c, inv = outputs(1)
        ptrs, cnt, off = triple([segs_of(d[0], (n // 3,))])
        return lib.esr_bucket_ids_by_owner_multi(ptrs, cnt, off, 2, world, lr.data_ptr(), p.data_ptr(), inv.data_ptr(),
                                                 c.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), lr, p, c, inv
    out["esr_bucket_ids_by_owner_multi"] = (lib.esr_bucket_workspace_bytes(n), multi, h[:1])

    for nb in (1, 2):
        def batched(ws, nbytes, nb=nb):
            lr, p, c, inv = outputs(nb)
            ptrs, cnt, off = triple([segs_of(d[b], (n // 3,)) for b in range(nb)])
            return lib.esr_bucket_ids_by_owner_batched(ptrs, cnt, off, 2, nb, world, lr.data_ptr(), p.data_ptr(),
                                                       inv.data_ptr(), c.data_ptr(), ws.data_ptr(), nbytes,
                                                       ops._stream()), lr, p, c, inv
        out["esr_bucket_ids_by_owner_batched/%d" % nb] = (lib.esr_bucket_batched_workspace_bytes(n, nb), batched, h[:nb])
    return out


def rows_calls(dev, rows):
    """esr_argsort_columns over `rows` columns of 2049 scores and esr_score_topk (k = 1025: the full sort) over `rows`
    queries: name -> (bytes needed, call(ws, ws_bytes) -> rc)"""
    from esrecsys_amd import _lib, ops
    lib = _lib.load()
    n, D, k = 2049, 32, 1025
    rng = np.random.default_rng(rows)
    scores = torch.from_numpy((rng.integers(-40, 41, (n, rows)) / 8.0).astype(np.float32)).to(dev)
    q = torch.from_numpy((rng.integers(-8, 9, (rows, D)) / 4.0).astype(np.float32)).to(dev)
    c = torch.from_numpy((rng.integers(-8, 9, (n, D)) / 4.0).astype(np.float32)).to(dev)
    hq, hc = q.cpu().numpy().astype(np.float64), c.cpu().numpy().astype(np.float64)

    def argsort(ws, nbytes):
        idx = torch.empty((n, rows), dtype=torch.int32, device=dev)
        rc = lib.esr_argsort_columns(scores.data_ptr(), n, rows, idx.data_ptr(), ws.data_ptr(), nbytes, ops._stream())
        return rc, lambda: np.array_equal(idx.cpu().numpy(), np.argsort(scores.cpu().numpy(), axis=0, kind="stable"))

    def topk(ws, nbytes):
        s = torch.empty((rows, k), dtype=torch.float32, device=dev)
        i = torch.empty((rows, k), dtype=torch.int32, device=dev)
        rc = lib.esr_score_topk(q.data_ptr(), c.data_ptr(), rows, n, D, k, s.data_ptr(), i.data_ptr(), ws.data_ptr(), nbytes,
                                ops._stream())
        # (multiples of 1/16 with |sum| < 2^7: every dot product is exact in f32, ties go to the lower index)
        return rc, lambda: np.array_equal(i.cpu().numpy(), np.argsort(-(hq @ hc.T), axis=1, kind="stable")[:, :k])

    return {"esr_argsort_columns": (lib.esr_argsort_columns_workspace_bytes(n, rows), argsort),
            "esr_score_topk": (lib.esr_score_topk_workspace_bytes(rows, n, k), topk)}


def refused(lib, name, rc):
    msg = lib.esr_last_error()
    print("%s: one byte short -> code %d, %r" % (name, rc, msg))
    return rc == EWORKSPACE and name.split("/")[0].encode() in msg


@pytest.mark.parametrize("n,V", SORT_CASES)
def test_sort_workspace_of_the_stated_size_is_enough(dev, n, V):
    for name, (need, call, h) in sort_calls(dev, n, V).items():
        rc, s, p = call(torch.empty(need, dtype=torch.uint8, device=dev), need)
        assert rc == 0, (name, rc)
        for b in range(h.shape[0]):
            es, ep = stable_sort(h[b])
            assert np.array_equal(s[b].cpu().numpy(), es) and np.array_equal(p[b].cpu().numpy(), ep), (name, b)


@pytest.mark.parametrize("n,V", SORT_CASES)
def test_sort_workspace_one_byte_short_is_refused(dev, n, V):
    from esrecsys_amd import _lib
    for name, (need, call, _) in sort_calls(dev, n, V).items():
        rc = call(torch.empty(need, dtype=torch.uint8, device=dev), need - 1)[0]
        assert refused(_lib.load(), name, rc), name


@pytest.mark.parametrize("n,world", BUCKET_CASES)
def test_bucket_workspace_of_the_stated_size_is_enough(dev, n, world):
    for name, (need, call, h) in bucket_calls(dev, n, world).items():
        rc, *got = call(torch.empty(need, dtype=torch.uint8, device=dev), need)
        assert rc == 0, (name, rc)
        for b in range(h.shape[0]):
            for g, e in zip(got, stable_bucket(h[b], world)):
                assert np.array_equal(g[b].cpu().numpy(), e), (name, b)


@pytest.mark.parametrize("n,world", BUCKET_CASES)
def test_bucket_workspace_one_byte_short_is_refused(dev, n, world):
    from esrecsys_amd import _lib
    for name, (need, call, _) in bucket_calls(dev, n, world).items():
        rc = call(torch.empty(need, dtype=torch.uint8, device=dev), need - 1)[0]
        assert refused(_lib.load(), name, rc), name


@pytest.mark.parametrize("rows", [1, 9])
def test_key_row_sorts_workspace_is_exact(dev, rows):
    """esr_argsort_columns and esr_score_topk sort rows of keys eight at a time (one row: as any list)"""
    from esrecsys_amd import _lib
    for name, (need, call) in rows_calls(dev, rows).items():
        rc, right = call(torch.empty(need, dtype=torch.uint8, device=dev), need)
        assert rc == 0 and right(), (name, rc)
        rc, _ = call(torch.empty(need, dtype=torch.uint8, device=dev), need - 1)
        assert refused(_lib.load(), name, rc), name


# segment lengths of lists of <= 3000 ids in 1 - 4 segments, with an empty first, middle and last segment: the slots
# behind the last segment, and an empty segment's pointer, are never read
SEGMENT_SHAPES = [(3000,), (1500, 1500), (0, 3000), (3000, 0), (1000, 0, 2000), (0, 0, 300), (700, 900, 0),
                  (800, 700, 600, 900), (0, 1000, 0, 1100), (300, 0, 0, 0), (0, 0, 0, 2500)]


@pytest.mark.parametrize("counts", SEGMENT_SHAPES, ids=lambda c: "-".join(map(str, c)))
def test_unused_segment_slots_do_not_matter(dev, counts):
    from esrecsys_amd import ops
    Vk, world = 700, 3                                    # rows per table: equal ids within and across segments
    n = sum(counts)
    h, d = ids_for(dev, 1, n, Vk)
    offsets = [Vk * i for i in range(len(counts))]
    segs = segs_of(d[0], np.cumsum(counts)[:-1])
    virt = h[0] + np.repeat(offsets, counts).astype(np.int32)
    s, p = ops.segment_sort_multi(segs, offsets, Vk * len(counts))
    es, ep = stable_sort(virt)
    assert np.array_equal(s.cpu().numpy(), es) and np.array_equal(p.cpu().numpy(), ep)
    got = ops.bucket_ids_by_owner(segs, world, want_inverse=True, offsets=offsets)
    for g, e in zip(got, stable_bucket(virt, world)):
        assert np.array_equal(g.cpu().numpy(), e)

"""GPU: the IVF search (esr_ivf_search, IVFIndex.search) bit for bit across its geometry -- esr_ivf.hip ivf_geom:
  pitch  = align_up(max(longest list, ceil((k + 1) / nprobe)), 64)    a (query, list) pair's dense score row
  f      = min(nprobe, max(k // pitch + 1, 8192 // pitch))            head probe slots, scored densely and selected
  rounds = ceil((nprobe - f) / 8)                                     filter rounds: scores >= tau appended, a lazy
                                                                      compaction (lists over mark = max(3 k, 1536)) between
  ppitch = max(k, mark) + min(8, nprobe - f) pitch                    a query's record list
  chunk  = min(nq, max(64, 2^31 // (4 f pitch + 8 ppitch)), (65 535 - nlist) 64 // max(f, 8))   queries per pass
test_gpu_ivf.py stays at nlist <= 128, nprobe <= 20 and one chunk; these cases reach nlist > 1024 (ivf_prep_kernel's
loop over lists), dozens of filter rounds, memory and grid-y chunking, a head that is streamed rather than cached in LDS,
empty probed lists, unions shorter than k, and the bench's own geometry through the k-means build.

Bar: integer-valued queries and candidates, so every f32 score is exact on the matrix cores and in NumPy alike.  The
answer is then fully specified: the k best of the union of the query's probed lists ordered by (score descending, probe
slot ascending, candidate row ascending) -- the select's composite orders by (score, lower slot * pitch + position), and a
list keeps its members in ascending row -- padded with -inf / -1.  Scores and indices must match it bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEL_LDS_WORDS = 8192      # esr_retrieve.hip kSelLdsWords: a dense head row longer than this is streamed, not cached
SEL_LDS_RECORDS = 4096    # ... and a record list longer than this in the tail select


def _cdiv(a, b):
    return -(-a // b)


def ivf_geom(nq, max_list, nprobe, k, nlist):
    """esr_ivf.hip ivf_geom restated, plus the counts a case is about (filter rounds, chunks)"""
    pitch = _cdiv(max(max_list, _cdiv(k + 1, nprobe)), 64) * 64
    f = min(nprobe, max(k // pitch + 1, 8192 // pitch))
    mark = max(3 * k, 1536)
    ppitch = max(k, mark) + min(8, nprobe - f) * pitch
    chunk = min(nq, max(64, 2 ** 31 // (f * pitch * 4 + ppitch * 8)))
    chunk = max(1, min(chunk, (65535 - nlist) * 64 // max(f, 8)))
    return dict(pitch=pitch, f=f, mark=mark, ppitch=ppitch, chunk=chunk, rounds=_cdiv(nprobe - f, 8),
                chunks=_cdiv(nq, chunk))


def ivf_workspace_bytes(g, nprobe, nlist, sort_ws_bytes):
    """esr_ivf.hip ivf_layout for one chunk of queries; sort_ws_bytes(n) = esr_segment_sort_workspace_bytes"""
    cq, f, pitch = g["chunk"], g["f"], g["pitch"]
    pm = cq * max(f, min(8, max(1, nprobe - f)))
    parts = [4 * pm] * 3 + [4 * (nlist + 1)] * 2 + [4 * cq * f * pitch, 8 * cq * g["ppitch"], 4 * cq, 4 * cq,
                                                    sort_ws_bytes(pm)]
    return sum(_cdiv(b, 256) * 256 for b in parts)


# (nq, max_list, nprobe, k, nlist) of the cases below and the regime each must reach; test_abi checks the restatement
# against the library's workspace query at these points
GEOMETRIES = {
    "small_lists_32768": ((128, 200, 700, 1000, 32768), dict(pitch=256, f=32, rounds=84, chunks=1)),
    "small_lists_4096": ((128, 200, 700, 1000, 4096), dict(pitch=256, f=32, rounds=84, chunks=1)),
    "giant_list": ((600, 300_000, 4, 1024, 101), dict(pitch=300_032, f=1, rounds=1, chunk=254, chunks=3)),
    "grid_y": ((40_000, 64, 160, 100, 4096), dict(pitch=64, f=128, rounds=4, chunk=30_719, chunks=2)),
    "short_union": ((64, 4, 200, 1024, 2048), dict(pitch=64, f=128, rounds=9, chunks=1)),
    "width_head_only": ((50, 300, 20, 10, 64), dict(pitch=320, f=20, rounds=0, chunks=1)),
    "width_filter": ((50, 300, 60, 300, 64), dict(pitch=320, f=25, rounds=5, chunks=1)),
}


def _check_regime(name, nq, max_list, nprobe, k, nlist, **want):
    g = ivf_geom(nq, max_list, nprobe, k, nlist)
    print("IVF case %s: nq %d nlist %d nprobe %d k %d -> pitch %d, f %d, filter rounds %d, chunks %d of %d queries, "
          "head row %d" % (name, nq, nlist, nprobe, k, g["pitch"], g["f"], g["rounds"], g["chunks"], g["chunk"],
                           g["f"] * g["pitch"]))
    for key, v in want.items():
        assert g[key] == v, (name, key, g[key], v)
    return g


def _hand_built(cands, assign, nlist):
    """an IVFIndex over an explicit assignment (no k-means), as IVFIndex.__init__ ends: the members of a list in
    ascending row (a stable sort), list_off, orig, cands_sorted, max_list.  Returns (index, list_off, orig) with the
    host copies.  It has no centroids: search it with probe_lists."""
    from esrecsys_amd.ivf import IVFIndex
    dev = torch.device("cuda", 0)
    orig = np.argsort(assign, kind="stable").astype(np.int64)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(assign, minlength=nlist))
    index = IVFIndex.__new__(IVFIndex)
    index.centroids = None
    index.list_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    index.orig = torch.from_numpy(orig.astype(np.int32)).to(dev)
    index.cands_sorted = torch.from_numpy(np.ascontiguousarray(cands[orig])).to(dev)
    index.nlist, index.N, index.D = nlist, cands.shape[0], cands.shape[1]
    index.max_list = int(np.diff(off).max())
    return index, off, orig


def _ints(rng, shape, lo=-4, hi=4):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _expected(srow, off, orig, lists, k):
    """the k best of the union of `lists` (probe slot order), srow = the query's scores of every candidate row:
    (score desc, slot asc, row asc), padded with -inf / -1"""
    rows = np.concatenate([orig[off[l]:off[l + 1]] for l in lists])
    slots = np.repeat(np.arange(len(lists)), [off[l + 1] - off[l] for l in lists])
    sc, n = srow[rows], len(rows)
    if n > k:   # (only what reaches the k-th best score can be in the answer: fewer rows to lexsort)
        keep = sc >= np.partition(sc, n - k)[n - k]
        rows, slots, sc = rows[keep], slots[keep], sc[keep]
    o = np.lexsort((rows, slots, -sc))[:k]
    es = np.full(k, -np.inf, np.float32)
    ei = np.full(k, -1, np.int32)
    es[:len(o)] = sc[o] + np.float32(0.0)   # (a -0 sum is +0 on the device)
    ei[:len(o)] = rows[o]
    return es, ei, n


def _assert_rows_exact(full, check_rows, off, orig, lists, k, gs, gi):
    """answer rows `check_rows` (gs, gi) against _expected bit for bit, full[j] = the scores of query check_rows[j];
    returns the union sizes"""
    sizes = []
    for j, r in enumerate(check_rows):
        es, ei, n = _expected(full[j], off, orig, lists[r], k)
        sizes.append(n)
        assert np.array_equal(gi[r], ei), ("indices", int(r), np.flatnonzero(gi[r] != ei)[:8], n)
        assert np.array_equal(gs[r].view(np.int32), es.view(np.int32)), ("scores", int(r), n)
    return sizes


def _assert_bit_exact(q, cands, off, orig, lists, k, gs, gi, check_rows):
    """_assert_rows_exact, the score rows computed on the host a block of queries at a time"""
    sizes = []
    block = max(1, 2 ** 25 // cands.shape[0])
    for b0 in range(0, len(check_rows), block):
        rb = check_rows[b0:b0 + block]
        full = q[rb] @ cands.T   # f32: integer-valued, so exact
        sizes += _assert_rows_exact(full, rb, off, orig, lists, k, gs, gi)
    return np.array(sizes)


def _search(index, q, k, lists):
    dev = torch.device("cuda", 0)
    s, i = index.search(torch.from_numpy(q).to(dev), k, lists.shape[1],
                        probe_lists=torch.from_numpy(np.ascontiguousarray(lists, np.int32)).to(dev))
    return s.cpu().numpy(), i.cpu().numpy()


def _skewed_assignment(rng, nlist, N, longest, empty_frac=0.2):
    """list of every row: about empty_frac of the lists empty, sizes skewed (exponential), one list exactly `longest`
    long; rows of a list scattered over the matrix"""
    nonempty = rng.permutation(nlist)[:nlist - int(empty_frac * nlist)]
    sizes = np.minimum(longest, 1 + rng.exponential(N / len(nonempty), len(nonempty)).astype(np.int64))
    sizes[0] = longest
    assign = rng.permutation(np.repeat(nonempty, sizes))
    return assign, np.setdiff1d(np.arange(nlist), nonempty)


@pytest.mark.parametrize("name,N,D", [("small_lists_32768", 500_000, 20), ("small_lists_4096", 200_000, 100)])
def test_ivf_many_small_lists_many_filter_rounds(dev, name, N, D):
    """nlist > 1024 (the prep kernel's loop over lists runs 32 or 4 times), skewed lists with ~20 % empty, longest 200:
    pitch 256, a head of 32 slots and 84 filter rounds of 8 at k = 1000, nprobe = 700.  Every fourth query's head slots
    are all empty lists (tau = -inf after the head: its list opens with k -inf records)."""
    (nq, longest, nprobe, k, nlist), want = GEOMETRIES[name]
    rng = np.random.default_rng(nlist + D)
    assign, empty = _skewed_assignment(rng, nlist, N, longest)
    cands = _ints(rng, (len(assign), D))
    q = _ints(rng, (nq, D))
    index, off, orig = _hand_built(cands, assign, nlist)
    assert index.max_list == longest and len(empty) > 0.15 * nlist and nlist > 1024
    g = _check_regime(name, nq, index.max_list, nprobe, k, nlist, **want)
    nonempty = np.setdiff1d(np.arange(nlist), empty)
    lists = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    for r in range(0, nq, 4):   # head slots: empty lists only; the rest non-empty ones
        lists[r, :g["f"]] = rng.choice(empty, g["f"], replace=False)
        lists[r, g["f"]:] = rng.choice(nonempty, nprobe - g["f"], replace=False)
    gs, gi = _search(index, q, k, lists)
    sizes = _assert_bit_exact(q, cands, off, orig, lists, k, gs, gi, np.arange(nq))
    print("  union sizes %d .. %d" % (sizes.min(), sizes.max()))
    assert sizes.min() > k


def test_ivf_one_giant_list_memory_chunks(dev):
    """One list of 300 000 rows and 100 of 1000: pitch 300 032 makes the head a single slot whose row (> 8192 scores)
    the head select streams, and the 2 GiB bound cuts 600 queries into chunks of 254, 254, 92.  Entries in {-1, 0, 1}
    at D = 32: scores in [-32, 32], ties by the thousand.  The giant list sits in slot 0 for a third of the queries (the
    head streams it), in slot 1 .. 3 for another third (the filter lets it through whole -- a head list of 1000 < k
    leaves tau = -inf -- and the tail select streams 300 000 records), and is absent for the rest."""
    (nq, longest, nprobe, k, nlist), want = GEOMETRIES["giant_list"]
    rng = np.random.default_rng(5)
    assign = rng.permutation(np.repeat(np.arange(nlist), [longest] + [1000] * (nlist - 1)))
    D = 32
    cands = _ints(rng, (len(assign), D), -1, 1)
    q = _ints(rng, (nq, D), -1, 1)
    index, off, orig = _hand_built(cands, assign, nlist)
    g = _check_regime("giant_list", nq, index.max_list, nprobe, k, nlist, **want)
    assert g["f"] * g["pitch"] > SEL_LDS_WORDS and g["ppitch"] > longest
    lists = np.stack([1 + rng.permutation(nlist - 1)[:nprobe] for _ in range(nq)])
    for r in range(nq):
        if r % 3 == 0:
            lists[r, 0] = 0
        elif r % 3 == 1:
            lists[r, 1 + (r // 3) % 3] = 0
    gs, gi = _search(index, q, k, lists)
    sizes = _assert_bit_exact(q, cands, off, orig, lists, k, gs, gi, np.arange(nq))
    assert (sizes > SEL_LDS_RECORDS + k).sum() >= nq // 3 * 2   # the giant list's queries: a streamed tail select


def test_ivf_grid_y_chunks(dev):
    """4096 lists of exactly 64 rows: a head of 128 slots makes the row tiles of a chunk's pairs (one grid dimension,
    <= 65 535) the bound -- 30 719 queries a chunk, two chunks for 40 000 queries; 4 filter rounds follow.  ~1000 queries
    checked: every one within 64 of the chunk boundary, the first, the last and the rest evenly spread."""
    (nq, longest, nprobe, k, nlist), want = GEOMETRIES["grid_y"]
    rng = np.random.default_rng(11)
    D = 16
    assign = rng.permutation(np.repeat(np.arange(nlist), longest))
    cands = _ints(rng, (len(assign), D))
    q = _ints(rng, (nq, D))
    index, off, orig = _hand_built(cands, assign, nlist)
    g = _check_regime("grid_y", nq, index.max_list, nprobe, k, nlist, **want)
    assert nlist > 1024
    # distinct lists per query: a + b j mod 4096 with b odd
    a = rng.integers(0, nlist, nq)[:, None]
    b = 2 * rng.integers(0, nlist // 2, nq)[:, None] + 1
    lists = (a + b * np.arange(nprobe)[None, :]) % nlist
    gs, gi = _search(index, q, k, lists)
    edge = g["chunk"]
    rows = np.unique(np.concatenate([np.arange(edge - 64, edge + 64), [0, nq - 1],
                                     np.linspace(0, nq - 1, 870).astype(np.int64)]))
    assert len(rows) >= 990
    _assert_bit_exact(q, cands, off, orig, lists, k, gs, gi, rows)


def test_ivf_union_shorter_than_k(dev):
    """Lists of at most 4 rows, 80 % empty: 200 probed lists hold at most 800 < k = 1024 candidates.  The head's tau is
    -inf, the filter rounds keep everything, and the answer is the whole union followed by exactly -inf / -1."""
    (nq, longest, nprobe, k, nlist), want = GEOMETRIES["short_union"]
    rng = np.random.default_rng(3)
    nonempty = rng.permutation(nlist)[:nlist // 5]
    sizes = rng.integers(1, longest + 1, len(nonempty))
    sizes[0] = longest
    assign = rng.permutation(np.repeat(nonempty, sizes))
    D = 36
    cands = _ints(rng, (len(assign), D))
    q = _ints(rng, (nq, D))
    index, off, orig = _hand_built(cands, assign, nlist)
    _check_regime("short_union", nq, index.max_list, nprobe, k, nlist, **want)
    lists = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    lists[1] = np.concatenate([rng.choice(np.setdiff1d(np.arange(nlist), nonempty), nprobe - 1, replace=False),
                               nonempty[:1]])   # one non-empty list, in the last slot
    gs, gi = _search(index, q, k, lists)
    sizes = _assert_bit_exact(q, cands, off, orig, lists, k, gs, gi, np.arange(nq))
    assert sizes.max() < k and sizes[1] == longest
    for r in range(nq):
        assert np.all(gi[r, sizes[r]:] == -1) and np.all(np.isneginf(gs[r, sizes[r]:]))
        assert np.all(gi[r, :sizes[r]] >= 0) and np.all(np.isfinite(gs[r, :sizes[r]]))


@pytest.mark.parametrize("D", [4, 20, 36, 100, 132])
@pytest.mark.parametrize("case", ["width_head_only", "width_filter"])
def test_ivf_width_sweep(dev, D, case):
    """D % 16 != 0 leaves the last LDS stage of the score kernel partly zero (4, 20, 36, 100, 132); head-only
    (nprobe <= f) and head + filter rounds, on a hand-built index of 64 lists (some empty, the longest 120)."""
    (nq, longest, nprobe, k, nlist), want = GEOMETRIES[case]
    rng = np.random.default_rng(D)
    assign, empty = _skewed_assignment(rng, nlist, 3000, longest, empty_frac=0.1)
    cands = _ints(rng, (len(assign), D))
    q = _ints(rng, (nq, D))
    index, off, orig = _hand_built(cands, assign, nlist)
    _check_regime("%s D=%d" % (case, D), nq, index.max_list, nprobe, k, nlist, **want)
    lists = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    others = rng.permutation(np.setdiff1d(np.arange(nlist), empty[:1]))
    lists[0] = np.concatenate([empty[:1], others[:nprobe - 1]])   # an empty list in the head slot
    lists[1] = np.concatenate([others[:nprobe - 1], empty[:1]])   # ... and in the last slot
    gs, gi = _search(index, q, k, lists)
    _assert_bit_exact(q, cands, off, orig, lists, k, gs, gi, np.arange(nq))


# ---- the bench's geometry through the real build ---------------------------------------------------------------------
BENCH_N, BENCH_D, BENCH_NQ = 1_048_576, 512, 8192
BENCH_LEGS = {1024: [(10, 8), (500, 32), (500, 128)], 4096: [(500, 16), (500, 64)]}


@pytest.fixture(scope="module")
def bench_corpus(dev):
    """bench_retrieve.measure_ivf's clustered corpus (4096 unit centres + N(0, 0.6^2 / D) noise) scaled by 1.5 sqrt(D)
    and rounded into [-4, 4]: integer-valued (|score| <= 16 D = 8192, every partial sum exact in f32), clusters kept.
    Also the full host score rows of 64 sampled queries (f32 BLAS: exact)."""
    g = torch.Generator(device=dev).manual_seed(1701)
    centres = torch.randn((4096, BENCH_D), generator=g, device=dev)
    centres /= centres.norm(dim=1, keepdim=True)

    def draw(n):
        x = centres[torch.randint(0, 4096, (n,), generator=g, device=dev)] + \
            torch.randn((n, BENCH_D), generator=g, device=dev) * (0.6 * BENCH_D ** -0.5)
        return (x * (1.5 * BENCH_D ** 0.5)).round_().clamp_(-4, 4).contiguous()

    c, q = draw(BENCH_N), draw(BENCH_NQ)
    qh = q.cpu().numpy()
    sample = np.unique(np.concatenate([[0, BENCH_NQ - 1], np.random.default_rng(9).choice(BENCH_NQ, 62, replace=False)]))
    full = qh[sample] @ c.cpu().numpy().T
    return c, q, sample, full


def _bench_properties(c, q, s, i, lists, list_of, block=256):
    """every query: scores non-increasing, -inf exactly where the index is -1 (at the end), indices unique and inside
    the probed lists, each score the exact dot product of its row (device f32 batched products of integer rows: exact)"""
    for r0 in range(0, q.shape[0], block):
        sb, ib, lb = s[r0:r0 + block], i[r0:r0 + block].long(), lists[r0:r0 + block].long()
        valid = ib >= 0
        assert torch.equal(valid, ~torch.isneginf(sb)) and bool((valid[:, 1:] <= valid[:, :-1]).all())
        assert bool((sb[:, 1:] <= sb[:, :-1]).all())
        srt = ib.sort(dim=1).values
        assert not bool(((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)).any())
        safe = ib.clamp(min=0)
        inside = (list_of[safe][:, :, None] == lb[:, None, :]).any(-1)
        assert bool((inside | ~valid).all())
        dots = torch.bmm(c[safe], q[r0:r0 + block, :, None])[..., 0]
        assert torch.equal(torch.where(valid, dots, sb), sb)


@pytest.mark.parametrize("nlist", sorted(BENCH_LEGS))
def test_ivf_bench_geometry_through_the_build(dev, bench_corpus, nlist):
    """IVFIndex(c, nlist) with its own k-means on the bench's corpus shape (N = 1 048 576, D = 512, nq = 8192) and the
    bench's (k, nprobe) legs: 64 sampled queries bit for bit, every query by the properties above.  The search without
    probe_lists must equal the search given the centroid probe explicitly, bit for bit."""
    from esrecsys_amd import ops
    from esrecsys_amd.ivf import IVFIndex
    c, q, sample, full = bench_corpus
    index = IVFIndex(c, nlist)
    off, orig = index.list_off.cpu().numpy().astype(np.int64), index.orig.cpu().numpy().astype(np.int64)
    list_of = torch.repeat_interleave(torch.arange(nlist, device=dev), index.list_off.diff().long())[
        torch.argsort(index.orig.long())]
    for k, nprobe in BENCH_LEGS[nlist]:
        g = _check_regime("bench nlist %d longest %d" % (nlist, index.max_list), BENCH_NQ, index.max_list, nprobe, k,
                          nlist)
        assert g["rounds"] >= _cdiv(nprobe - 8192 // (BENCH_N // nlist), 8)   # (the longest list >= the mean)
        _, lists = ops.retrieve_topk(q, index.centroids, nprobe, mode="exact")
        s, i = index.search(q, k, nprobe)
        s2, i2 = index.search(q, k, nprobe, probe_lists=lists)
        assert torch.equal(i, i2) and torch.equal(s.view(torch.int32), s2.view(torch.int32))
        _bench_properties(c, q, s, i, lists, list_of)
        gs, gi, hl = s.cpu().numpy(), i.cpu().numpy(), lists.cpu().numpy()
        sizes = _assert_rows_exact(full, sample, off, orig, hl, k, gs, gi)
        print("  k %d nprobe %d: union sizes %d .. %d" % (k, nprobe, min(sizes), max(sizes)))


def test_ivf_probe_lists_are_checked(dev):
    """search(probe_lists=...) takes an int32 [nq, nprobe] device tensor, 1 <= nprobe <= nlist"""
    rng = np.random.default_rng(1)
    cands, q = _ints(rng, (500, 8)), _ints(rng, (6, 8))
    index, _, _ = _hand_built(cands, rng.integers(0, 10, 500), 10)
    qd = torch.from_numpy(q).to(dev)
    lists = torch.arange(4, dtype=torch.int32, device=dev).repeat(6, 1)
    s, i = index.search(qd, 5, 4, probe_lists=lists)
    assert s.shape == i.shape == (6, 5)
    with pytest.raises(TypeError, match="probe_lists"):
        index.search(qd, 5, 4, probe_lists=lists.long())
    with pytest.raises(TypeError, match="probe_lists"):
        index.search(qd, 5, 4, probe_lists=lists.cpu())
    with pytest.raises(ValueError, match="probe_lists"):
        index.search(qd, 5, 3, probe_lists=lists)
    with pytest.raises(ValueError, match="probe_lists"):
        index.search(qd, 5, 4, probe_lists=lists[:5])
    with pytest.raises(ValueError, match="probe_lists"):
        index.search(qd, 5, 11, probe_lists=torch.zeros((6, 11), dtype=torch.int32, device=dev))

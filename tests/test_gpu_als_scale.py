"""GPU: esr_als.hip past one launch grid, one workgroup round and one unrolled loop.

Every grid-stride loop of the six kernels goes round at least twice here, so a wave and a workgroup solve a second row in
the LDS slot the first one used; the 4-way loop of als_long_rows runs with and without a tail, and the fp64 segment sum of
als_gram runs its 8-way loop thousands of times.  Rows are copies of a few prototype rows on the exact tables of
tests/_als_exact.py: a row's output depends on its own ratings only, so the expected bits of every copy are the prototype's,
computed by the CPU oracle (the Cholesky of the contract on the correctly rounded fma over exact sums) -- nothing is
compared with the code under test alone.  One row of the second round reads a NaN factor row that nobody else reads: it is
refused (fill value kept, failed == 1) and every other row keeps its bits."""
import numpy as np
import pytest
import torch

import _als_exact as ex
import _als_ref as ref

pytestmark = pytest.mark.gpu
GRID_CAP = 256 * 8   # esr_common.h kMaxGrid: the launchers' grid cap; more units go round the grid-stride loops
BLOCK = 256          # esr_common.h kBlock: threads per workgroup of als_predict
N_OTHER = ex.N_OTHER
FILL = 7.0
REG, WEIGHTED = 0.1, True


def geometry():
    from esrecsys_amd import ops
    return ops.als_geometry()


def class_lengths(cls):
    """About eight prototype lengths per row class (equal lengths get distinct content)."""
    C, W = geometry()
    return {1: [0, 1, 2, C - 1, C, 1, 2, C],
            2: [C + 1, 2 * C + 1, C * W, C + 1, 2 * C + 1, C * W, 3 * C - 1, C * W - 1],
            # 16 C + 1: 17 chunks; 21 chunks: the 4-way loop runs 5 full rounds, no tail; 23 chunks: a tail of two
            3: [C * W + 1, 16 * C + 1, 21 * C, 23 * C, 16 * C + 1, 16 * C + 1, 16 * C + 1, 16 * C + 1]}[cls]


_protos = {}


def prototypes(cls, rank, implicit):
    """(Y with one more, NaN, row; offsets, cols, values, expected rows) of a class's prototype rows.  Made once."""
    key = (cls, rank, implicit)
    if key not in _protos:
        rng = np.random.default_rng(9000 + 100 * cls + 2 * rank + implicit)
        Y = ex.table(rank, seed=5)
        offsets, cols, v = ex.make_rows(rng, class_lengths(cls), implicit)
        G, _ = ex.int_gram(Y)
        want, failures, bound = ex.oracle_rows(Y, offsets, cols, v, REG, WEIGHTED, implicit, FILL, G.astype(np.float32))
        ex.assert_exact(bound)
        assert failures == 0
        Yn = np.concatenate([Y, np.full((1, rank), np.nan, np.float32)])       # row N_OTHER: read by the planted row only
        _protos[key] = (Yn, offsets, cols, v, want)
    return _protos[key]


def zero_last(Yn):
    """The table whose Gram the implicit solve gets: the NaN row as zeros, which adds nothing."""
    Z = Yn.copy()
    Z[-1] = 0
    return Z


def run_class(dev, cls, rank, implicit, n_rows, second_round_from):
    """n_rows shuffled copies of the class's prototypes: a clean call, then the same call with one refused row."""
    Yn, p_off, p_cols, p_v, p_want = prototypes(cls, rank, implicit)
    rng = np.random.default_rng(cls)
    which = rng.permutation(n_rows) % (len(p_off) - 1)
    offsets, cols, v = ex.tile_rows(p_off, p_cols, p_v, which)
    want = p_want[which]
    gram_of = zero_last(Yn)
    out, word = ex.solve(dev, Yn, offsets, cols, v, REG, WEIGHTED, implicit, FILL, gram_of=gram_of)
    assert word == 0
    assert np.array_equal(ex.bits(out.cpu().numpy()), ex.bits(want))
    # the refused row: in the second grid round, with at least one rating; its first rating moves to the NaN row
    lens = np.diff(offsets)
    victim = second_round_from + int(np.argmax(lens[second_round_from:] > 0))
    assert victim >= second_round_from and lens[victim] > 0
    cols = cols.copy()
    cols[offsets[victim]] = N_OTHER
    out, word = ex.solve(dev, Yn, offsets, cols, v, REG, WEIGHTED, implicit, FILL, gram_of=gram_of)
    want = want.copy()
    want[victim] = FILL
    assert word == 1
    assert np.array_equal(ex.bits(out.cpu().numpy()), ex.bits(want))
    return offsets


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", [5, 64])
def test_wave_rows_past_one_grid(dev, rank, implicit):
    C, W = geometry()
    n_rows = GRID_CAP * W + 5                      # als_wave_rows: W rows per workgroup, GRID_CAP workgroups
    assert max(class_lengths(1)) <= C and n_rows > GRID_CAP * W
    if rank == 64:                                 # the request above the 64 KiB a kernel gets unasked
        assert 4 * W * (rank * (rank | 1) + 64) == 67584
    run_class(dev, 1, rank, implicit, n_rows, GRID_CAP * W)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", [5, 64])
def test_group_rows_past_one_grid(dev, rank, implicit):
    C, W = geometry()
    n_rows = GRID_CAP + 3                          # als_group_rows: a workgroup per row
    assert C < min(class_lengths(2)) and max(class_lengths(2)) <= C * W and n_rows > GRID_CAP
    run_class(dev, 2, rank, implicit, n_rows, GRID_CAP)


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", [5, 33])
def test_long_rows_past_one_grid(dev, rank, implicit):
    from esrecsys_amd import ops
    C, W = geometry()
    n_rows = GRID_CAP + 3                          # als_long_rows: a workgroup per row; als_chunk_partials: a wave per chunk
    lens = np.array(class_lengths(3))
    assert min(lens) > C * W and n_rows > GRID_CAP
    assert sorted(set((-(-lens // C)).tolist())) == [5, 17, 21, 23]
    which = np.random.default_rng(3).permutation(n_rows) % len(lens)           # run_class draws the same
    chunks = int((-(-lens[which] // C)).sum())
    assert chunks > 4 * GRID_CAP * W               # als_chunk_partials: 4 x GRID_CAP workgroups of W waves
    nnz = int(lens[which].sum())
    need = chunks * (rank * rank + rank) * 4       # the chunk partials alone: 156 MB at rank 33; the lists come on top
    have = int(ops._lib.load().esr_als_solve_workspace_bytes(n_rows, nnz, rank))
    assert have > need, (have, need)
    offsets = run_class(dev, 3, rank, implicit, n_rows, GRID_CAP)
    assert int(offsets[-1]) == nnz


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
def test_mixed_classes_and_launch_cuts(dev, implicit):
    """All three classes in one call, each past its threshold, the rows interleaved; then the same rows in four calls whose
    cuts fall inside every class: equal bits, and the oracle's."""
    C, W = geometry()
    rank = 5
    counts = {1: GRID_CAP * W + 5, 2: GRID_CAP + 3, 3: GRID_CAP + 3}
    parts = [prototypes(cls, rank, implicit) for cls in (1, 2, 3)]
    Yn = parts[0][0]
    assert all(np.array_equal(p[0], Yn, equal_nan=True) for p in parts)
    base = np.concatenate([[0], np.cumsum([len(p[1]) - 1 for p in parts])])      # prototype index of each class's first
    p_off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[1]) for p in parts]))]).astype(np.int64)
    p_cols, p_v = np.concatenate([p[2] for p in parts]), np.concatenate([p[3] for p in parts])
    p_want = np.concatenate([p[4] for p in parts])
    rng = np.random.default_rng(12)
    which = np.concatenate([base[q] + rng.permutation(counts[cls]) % (len(parts[q][1]) - 1) for q, cls in enumerate((1, 2, 3))])
    which = which[rng.permutation(len(which))]
    lens = np.diff(p_off)[which]
    n_rows = len(which)
    chunks3 = int((-(-lens[lens > C * W] // C)).sum())
    assert (lens <= C).sum() > GRID_CAP * W and ((lens > C) & (lens <= C * W)).sum() > GRID_CAP
    assert (lens > C * W).sum() > GRID_CAP and chunks3 > 4 * GRID_CAP * W
    offsets, cols, v = ex.tile_rows(p_off, p_cols, p_v, which)
    gram_of = zero_last(Yn)
    full, word = ex.solve(dev, Yn, offsets, cols, v, REG, WEIGHTED, implicit, FILL, gram_of=gram_of)
    assert word == 0
    assert np.array_equal(ex.bits(full.cpu().numpy()), ex.bits(p_want[which]))
    cuts = [0, n_rows // 4, n_rows // 2, 3 * n_rows // 4, n_rows]
    for a, b in zip(cuts, cuts[1:]):              # every piece holds rows of every class
        assert len(set(np.searchsorted([C + 1, C * W + 1], lens[a:b], side="right").tolist())) == 3
    pieces = torch.full_like(full, FILL)
    for a, b in zip(cuts, cuts[1:]):
        _, word = ex.solve(dev, Yn, offsets, cols, v, REG, WEIGHTED, implicit, FILL, a, b, out=pieces, gram_of=gram_of)
        assert word == 0
    assert torch.equal(pieces, full)


def test_gram_past_one_grid(dev):
    from esrecsys_amd import ops
    C, W = geometry()
    S = ops.als_gram_geometry()
    rank = 2
    n_seg = 4 * GRID_CAP * W + 3                   # als_gram_segments: 4 x GRID_CAP workgroups of W waves, a wave per segment
    n = (n_seg - 1) * S + 3                        # the last segment: three rows, an odd tail
    assert -(-n // S) == n_seg > 4 * GRID_CAP * W and n_seg >= 8 and n_seg % 8 == 3
    assert 4 * S < 2 ** 24                         # a segment's chain is exact; the fp64 sum of all segments is exact too
    t = torch.from_numpy(np.random.default_rng(21).integers(-2, 3, (n, rank), dtype=np.int8)).to(dev)
    Y = t.to(torch.float32)
    t64 = t.to(torch.float64)                      # the integer Gram: every fp64 sum of integers below 2^53 is exact
    want = (t64.t() @ t64).cpu().numpy()
    assert 2 ** 24 < want[0, 0] < 2 ** 53 and np.array_equal(want, np.rint(want))          # ... and float32 does round it
    got = ops.als_gram(Y).cpu().numpy()
    assert np.array_equal(ex.bits(got), ex.bits(want.astype(np.float32)))


def test_predict_past_one_grid(dev):
    from esrecsys_amd import ops
    rank, nu, ni = 5, 300, 120
    nq = GRID_CAP * BLOCK + 7
    rng = np.random.default_rng(31)
    X = rng.standard_normal((nu, rank)).astype(np.float32)
    Y = rng.standard_normal((ni, rank)).astype(np.float32)
    c = rng.standard_normal(nu)
    upos = rng.integers(0, nu, nq).astype(np.int32)
    ipos = rng.integers(0, ni, nq).astype(np.int32)
    unknown_u, unknown_i = rng.random(nq) < 0.01, rng.random(nq) < 0.01
    upos[unknown_u] = rng.choice(np.array([-1, nu, 2 ** 31 - 1], np.int32), int(unknown_u.sum()))
    ipos[unknown_i] = rng.choice(np.array([-1, ni, 2 ** 31 - 1], np.int32), int(unknown_i.sum()))
    upos[-1], ipos[-2] = nu, -1                    # in the second round for certain
    first, second = slice(0, GRID_CAP * BLOCK), slice(GRID_CAP * BLOCK, nq)
    unknown = (upos < 0) | (upos >= nu) | (ipos < 0) | (ipos >= ni)
    assert nq > GRID_CAP * BLOCK and unknown[first].any() and unknown[second].any() and not unknown[second].all()
    u0, i0 = np.where(unknown, 0, upos).astype(np.int64), np.where(unknown, 0, ipos).astype(np.int64)
    value = c[u0] + ref.dot64(X, Y, u0, i0)        # fp64, as the kernel: offset[u] + the dot product in ascending d
    d = (rng.integers(1, 11, nq) * 0.5).astype(np.float32)
    predicted = ref.predict(X, Y, np.where(unknown, -1, upos), np.where(unknown, -1, ipos), c)
    assert np.array_equal(ex.bits(predicted)[~unknown], ex.bits(value.astype(np.float32))[~unknown])
    for targets, want in ((None, predicted), (d, (d.astype(np.float64) - value).astype(np.float32))):
        got = ops.als_predict(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), torch.from_numpy(upos).to(dev),
                              torch.from_numpy(ipos).to(dev), torch.from_numpy(c).to(dev),
                              None if targets is None else torch.from_numpy(targets).to(dev)).cpu().numpy()
        assert np.array_equal(np.isnan(got), unknown)
        assert np.array_equal(ex.bits(got)[~unknown], ex.bits(want)[~unknown])

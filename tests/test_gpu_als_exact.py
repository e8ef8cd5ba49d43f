"""GPU: both ALS solves and the whole-table Gram of esr_als.hip against their restatement BIT FOR BIT.

Exact tables (tests/_als_exact.py): every sum in front of the Cholesky is exact in float32 whatever its order, so the output
row must equal ``_als_ref.cholesky_solve32`` on the correctly rounded fma in every bit -- lam, the diagonal add, the
left-looking Cholesky, both solves, the tile and lane mapping, the tails and the chunk sums are all pinned, independent of
how the matrix instruction rounds inside.

Random tables and planted order witnesses: the order contract itself -- a Gram entry is ONE k-ordered float32 fma chain per
chunk (per segment), the right-hand side is the even chain plus the odd chain, chunks add up in ascending order in float32,
segments in fp64 -- against ``_als_ref`` / ``_ials_ref`` on ``fma32_exact``.  A witness is one dimension whose three
non-zero squares are (1, 1, 2^24) in one order and (2^24, 1, 1) in the other: 2 + 2^24 is a float32, 2^24 + 1 is a tie that
falls back to 2^24, so the two orders differ in the restatement (asserted on the CPU first) and a kernel that took another
order cannot equal both."""
import numpy as np
import pytest
import torch

import _als_exact as ex
import _als_ref as ref
import _ials_ref as iref
import test_gpu_als as explicit_tests
import test_gpu_ials as implicit_tests

pytestmark = pytest.mark.gpu
N_OTHER = ex.N_OTHER
RANKS = [1, 2, 5, 31, 32, 33, 63, 64]
FILL = 7.0
EXACT = ref.fma32_exact


def geometry():
    from esrecsys_amd import ops
    return ops.als_geometry()


def segment():
    from esrecsys_amd import ops
    return ops.als_gram_geometry()


# ---- exact tables: the solve ---------------------------------------------------------------------------------------------
_exact = {}


def exact_problem(rank, implicit):
    """The lengths of test_gpu_als.lengths() and four more rows: fewer ratings than the rank (singular without lam), all
    ratings on one column, the first and the last column, and the last column alone.  Made once and never changed."""
    if (rank, implicit) not in _exact:
        rng = np.random.default_rng(3000 + 2 * rank + implicit)
        short = rng.permutation(N_OTHER)[:max(rank - 1, 1)]
        special = [short, [13] * 9, [0, N_OTHER - 1], [N_OTHER - 1]]
        Y = ex.table(rank)
        _exact[(rank, implicit)] = (Y,) + ex.make_rows(rng, explicit_tests.lengths(), implicit, special=special)
    return _exact[(rank, implicit)]


@pytest.mark.parametrize("reg", [0.1, 1e-3])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", RANKS)
def test_exact_rows_bit_for_bit(dev, rank, implicit, weighted, reg):
    Y, offsets, cols, v = exact_problem(rank, implicit)
    G, _ = ex.int_gram(Y)
    want, failures, bound = ex.oracle_rows(Y, offsets, cols, v, reg, weighted, implicit, FILL, G.astype(np.float32))
    ex.assert_exact(bound)                                                    # before any launch
    assert failures == 0 and len(offsets) - 1 == 16
    out, word = ex.solve(dev, Y, offsets, cols, v, reg, weighted, implicit, FILL)
    got = out.cpu().numpy()
    bad = [(r, int(offsets[r + 1] - offsets[r])) for r in range(len(want)) if not np.array_equal(ex.bits(got[r]), ex.bits(want[r]))]
    assert word == 0 and not bad, "rows (index, length) that differ from the oracle: %s" % bad


# ---- exact tables: the whole-table Gram and fold-in -----------------------------------------------------------------------
@pytest.mark.parametrize("rank", RANKS)
def test_exact_gram_bit_for_bit(dev, rank):
    from esrecsys_amd import ops
    S = segment()
    sizes = [0, 1, S - 1, S, S + 1, 8 * S, 8 * S + 1, 17 * S + 3]
    assert -(-sizes[-3] // S) == 8 and -(-sizes[-2] // S) == 9 and -(-sizes[-1] // S) == 18     # 8-way loop: alone, + 1, 2 x + 2
    Y = ex.table(rank, seed=1, n=sizes[-1])
    for n in sizes:
        G, largest = ex.int_gram(Y[:n])
        assert largest < 2 ** 24
        got = ops.als_gram(torch.from_numpy(Y[:n]).to(dev)).cpu().numpy()
        assert np.array_equal(ex.bits(got), ex.bits(G.astype(np.float32))), (rank, n)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("rank", [5, 33])
def test_exact_fold_in_bit_for_bit(dev, rank, weighted):
    from esrecsys_amd.factorization import ImplicitALS
    reg = 0.1
    items = np.arange(N_OTHER, dtype=np.int64) * 2 + 5
    m = ImplicitALS(np.zeros(N_OTHER, np.int64), items, rank=rank, reg=reg, alpha=0.5, weighted_reg=weighted, device=dev)
    Y = ex.table(rank, seed=2)
    m.item_factors.copy_(torch.from_numpy(Y))
    rng = np.random.default_rng(40 + rank)
    pos = rng.permutation(N_OTHER)[:rank + 7]
    doc = np.concatenate([items[pos], items[pos[:5]], [4, 10 ** 6]])            # five ids twice, two unknown ids
    strengths = rng.integers(1, 21, len(doc)).astype(np.float64)                # w = 0.5 x the summed strengths <= 20
    got = m.fold_in(doc, np.array([0, len(doc)], np.int64), strengths=strengths).cpu().numpy()
    d, i, w = iref.sum_events(np.zeros(len(doc) - 2, np.int64), np.concatenate([pos, pos[:5]]), strengths[:-2], 0.5)
    G, _ = ex.int_gram(Y)
    want, failures, bound = ex.oracle_rows(Y, np.array([0, len(i)]), i, w, reg, weighted, True, FILL, G.astype(np.float32))
    ex.assert_exact(bound)
    assert failures == 0 and np.array_equal(ex.bits(got), ex.bits(want))


# ---- random tables: the order contract --------------------------------------------------------------------------------------
def ulps(a, b):
    """The largest distance of two float32 arrays in units in the last place (of the ordered integer line)."""
    def line(x):
        i = ex.bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return int(np.max(np.abs(line(a) - line(b)))) if np.size(a) else 0


def random_gram(dev, rank, n):
    from esrecsys_amd import ops
    Y = implicit_tests.table(rank)[:n]
    return ops.als_gram(torch.from_numpy(Y).to(dev)).cpu().numpy(), iref.gram32(Y, segment(), fma=EXACT)


def random_rows(dev, rank, implicit, reg=0.1, weighted=True):
    """(kernel rows, restatement rows on the exact fma) of the bound tests' own problem(rank)."""
    C = geometry()[0]
    if implicit:
        offsets, cols, v, Y, _, _ = implicit_tests.problem(rank)
        G = iref.gram32(Y, segment(), fma=EXACT)
    else:
        offsets, cols, v, Y = explicit_tests.problem(rank)
    out, word = ex.solve(dev, Y, offsets, cols, v, reg, weighted, implicit, FILL)
    assert word == 0
    want = np.zeros((len(offsets) - 1, rank), np.float32)
    for r in range(len(want)):
        a, e = int(offsets[r]), int(offsets[r + 1])
        want[r] = (iref.solve_row32(Y, cols[a:e], v[a:e], G, reg, weighted, C, fma=EXACT) if implicit
                   else ref.solve_row32(Y, cols[a:e], v[a:e], reg, weighted, C, fma=EXACT))
    return out.cpu().numpy(), want


@pytest.mark.parametrize("rank", [1, 5, 32, 33, 64])
def test_random_gram_is_the_stated_chain(dev, rank):
    S = segment()
    for n in (1, 2, 65, S, S + 1, 2 * S + 3):
        got, want = random_gram(dev, rank, n)
        assert np.array_equal(ex.bits(got), ex.bits(want)), (rank, n, ulps(got, want))


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("rank", [1, 5, 32, 33, 64])
def test_random_rows_are_the_stated_chain(dev, rank, implicit):
    got, want = random_rows(dev, rank, implicit)
    bad = [(r, ulps(got[r], want[r])) for r in range(len(want)) if not np.array_equal(ex.bits(got[r]), ex.bits(want[r]))]
    assert not bad, "rows (index, ulps) that differ from the restatement: %s" % bad


# ---- planted order witnesses ------------------------------------------------------------------------------------------------
W_RANK, W_PAD = 5, 10      # table rows 0 .. 9: dimension 0 is zero (they pad a row); 10, 11: small; 12: big


def witness_table(small, big):
    Y = ex.table(W_RANK, seed=3, n=W_PAD + 3)
    Y[:W_PAD, 0] = 0
    Y[W_PAD:, 0] = [small, small, big]
    Y[W_PAD + 2, 1:] = 0           # the big row carries dimension 0 alone: every other sum stays small and exact
    return Y


def placements():
    C, W = geometry()
    return [("inside a chunk, across three gathers of 64", C - 3, (5, 70, 200)),
            ("across the even and odd halves", 9, (0, 2, 3)),
            ("across a chunk boundary, workgroup row", C + 5, (C - 1, C, C + 1)),
            ("across a chunk boundary, long row", C * W + 9, (2 * C - 1, 2 * C, 2 * C + 1))]


def witness_problem(kind, implicit):
    """(Y, offsets, cols, values): per placement one row with (small, small, big) at its three positions and one with
    (big, small, small); every other rating is on a padding row of the table."""
    small, big, v_small, v_big = {("gram", False): (1.0, 4096.0, 1.0, 1.0), ("gram", True): (1.0, 4096.0, 1.0, 1.0),
                                  ("rhs", False): (1.0, 4096.0, 1.0, 4096.0),          # d y = 1, 1, 2^24
                                  ("rhs", True): (0.5, 2.0 ** 23, 1.0, 1.0)}[(kind, implicit)]   # (1 + w) y = 1, 1, 2^24
    Y = witness_table(small, big)
    rng = np.random.default_rng(77)
    rows, vals = [], []
    for _, length, at in placements():
        for order in ((W_PAD, W_PAD + 1, W_PAD + 2), (W_PAD + 2, W_PAD, W_PAD + 1)):
            c = rng.integers(0, W_PAD, length)
            v = ex.values(rng, length, implicit)
            for p, col in zip(at, order):
                c[p], v[p] = col, (v_big if col == W_PAD + 2 else v_small)
            rows.append(c), vals.append(v)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return Y, offsets, np.concatenate(rows).astype(np.int32), np.concatenate(vals).astype(np.float32)


def witness_rows(dev, kind, implicit, reg=0.1, weighted=False):
    """(kernel rows, restatement rows); asserts on the CPU that the restatement tells the two orders apart."""
    C = geometry()[0]
    Y, offsets, cols, v = witness_problem(kind, implicit)
    G = iref.gram32(Y, segment(), fma=EXACT) if implicit else None
    want = np.zeros((len(offsets) - 1, W_RANK), np.float32)
    for r in range(len(want)):
        a, e = int(offsets[r]), int(offsets[r + 1])
        want[r] = (iref.solve_row32(Y, cols[a:e], v[a:e], G, reg, weighted, C, fma=EXACT) if implicit
                   else ref.solve_row32(Y, cols[a:e], v[a:e], reg, weighted, C, fma=EXACT))
    for p, (name, _, _) in enumerate(placements()):
        a0, a1, a2 = (int(offsets[2 * p + q]) for q in range(3))
        part = [(iref.gram_rhs32 if implicit else ref.gram_rhs32)(Y, cols[a:e], v[a:e], C, fma=EXACT)
                for a, e in ((a0, a1), (a1, a2))]
        entry = [(g[0, 0], b[0]) for g, b in part]
        which = 0 if kind == "gram" else 1
        assert {float(entry[0][which]), float(entry[1][which])} == {2.0 ** 24, 2.0 ** 24 + 2}, (name, entry)
    out, word = ex.solve(dev, Y, offsets, cols, v, reg, weighted, implicit, FILL)
    assert word == 0
    return out.cpu().numpy(), want


@pytest.mark.parametrize("implicit", [False, True], ids=["explicit", "implicit"])
@pytest.mark.parametrize("kind", ["gram", "rhs"])
def test_order_witnesses_in_the_row_solve(dev, kind, implicit):
    got, want = witness_rows(dev, kind, implicit)
    names = [name + (", ascending" if q == 0 else ", descending") for name, _, _ in placements() for q in range(2)]
    bad = [(names[r], ulps(got[r], want[r])) for r in range(len(want)) if not np.array_equal(ex.bits(got[r]), ex.bits(want[r]))]
    assert not bad, "witness rows that differ from the restatement: %s" % bad


def gram_witnesses():
    """[(name, table)]: the three witness rows inside one segment and across a segment boundary, in both orders; the other
    rows have dimension 0 zero."""
    S = segment()
    out = []
    for name, at in (("inside a segment", (5, 70, 300)), ("across a segment boundary", (S - 1, S, S + 1))):
        for q, order in enumerate(((1.0, 1.0, 4096.0), (4096.0, 1.0, 1.0))):
            Y = ex.table(W_RANK, seed=4, n=2 * S + 5)
            Y[:, 0] = 0
            for p, y0 in zip(at, order):
                Y[p, 0] = y0
                if y0 > 1:
                    Y[p, 1:] = 0
            out.append((name + (", ascending" if q == 0 else ", descending"), Y))
    return out


def test_order_witnesses_in_the_whole_table_gram(dev):
    from esrecsys_amd import ops
    cases = gram_witnesses()
    want = [iref.gram32(Y, segment(), fma=EXACT) for _, Y in cases]
    for p in (0, 2):          # a segment is one float32 chain; segments add up in fp64 and round once
        assert {float(want[p][0, 0]), float(want[p + 1][0, 0])} == {2.0 ** 24, 2.0 ** 24 + 2}, cases[p][0]
    for (name, Y), g in zip(cases, want):
        got = ops.als_gram(torch.from_numpy(Y).to(dev)).cpu().numpy()
        assert np.array_equal(ex.bits(got), ex.bits(g)), (name, ulps(got, g))

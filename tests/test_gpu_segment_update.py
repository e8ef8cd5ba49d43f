"""GPU: the row-sparse update engine (esr_optim.hip: segment_update_kernel / segment_long_kernel<VEC, NCH, OP>) in every
row geometry and under every op.

Section 1 pins the run sum BIT FOR BIT (kToDense) in all six <VEC, NCH> instantiations, at the positions where the
chunking, the four-in-flight loops, the `used` clamp, the K count and the grid cap change behaviour.  Section 2 runs
every op on every instantiation against float64.  Section 3: fused tables (1 .. 4).  Section 4: two argument checks.

Every table / accumulator / trace / output is the [8 : V + 8] view of a V + 16-row allocation with canary rows (Guarded):
after every call the canaries and every row without an occurrence must hold the bits they held before.
(ops.segment_sum_rows allocates its own output: compared in full, no canaries.)

bf16 tables: rel_err <= 2^-8 against float64 and the share of elements equal to the float64 answer rounded to bf16 (RNE)
above 0.999 -- the bars of test_sparse_adagrad_bf16_table, held over the whole table as there and over the TOUCHED rows
alone (untouched rows would dilute the share; they are also compared bit for bit).  Below 1000 touched elements that
reads "no element off".  A `same` list touches one row: at D = 1 and D = 3 it is applied to 64 / 22 start tables so that
64 touched elements are seen, and every case asserts that at least 8 of its touched elements round UP (a store that
truncates cannot pass).  What the inputs alone cost, measured on the CPU before any GPU run with a plain
float32 numpy restatement of both ops (run sums by expected_run_sums, w - lr * g and adagrad in float32, one RNE to
bf16) against the float64 answer on exactly the lists / rows / tables of _case (40 lists: 10 widths x 4 kinds; `same` =
1500 occurrences of one row): the share of touched-row elements equal is 1.0 in 29 of the 40 SGD lists and 24 of the 40
Adagrad lists, and at least 0.99998 (SGD; 516-uniform) and 0.99994 (Adagrad; 64-zipf, one element of 17 600) in the others
-- every one above the 0.9995 asked of the inputs; every `same` list (all start tables at D = 1 and 3 pooled): 1.0.  The float32 restatement is within 5.4e-8
(SGD) and 5.5e-8 (Adagrad; its accumulator 3.8e-7) of float64 by rel_err.  Measured on an MI355X: bf16 rel_err at most
3.6e-3 (Adagrad) / 2.9e-3 (SGD) against 2^-8 = 3.9e-3; f32 tables at most 3.8e-7 (Adagrad accumulator), 5.2e-8 (SGD),
2.7e-7 (momentum) against TOL = 1e-5.
"""
import functools

import numpy as np
import pytest
import torch

from _segment_sum_ref import (CHUNK, MAX_GRID, assert_pattern, expected_run_sums, geom, length_for_parts, nparts,
                              run_pattern, runs_of)
from conftest import rel_err
from oracle import optim as o_optim
from oracle import spotify as o_spotify

pytestmark = pytest.mark.gpu
TOL = 1e-5  # fp32 tolerance stated by north_star (tests/test_gpu_kernels.py)
F64 = np.float64
F32 = np.float32
GUARD = 8   # rows: keeps the view 16-byte aligned for every D and both dtypes

S1_WIDTHS = [1, 2, 3, 4, 8, 63, 64, 65, 100, 127, 130, 192, 193, 255, 256, 260, 512, 516, 768, 772, 1024]
S2_WIDTHS = [1, 3, 64, 65, 130, 255, 256, 260, 516, 1024]
REFUSED = [257, 258, 1028]
ALIGNS = (0, 1, 31)
SHORT_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97)
KINDS = ("uniform", "zipf", "same", "pattern")


def T(x, dev, dtype=None):
    t = torch.from_numpy(np.require(x, requirements="CW")).to(dev)  # (the shared arrays of _case are read-only: copied)
    return t.to(dtype) if dtype is not None else t


def N(t):
    return t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy()


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Guarded:
    """`view` = rows [GUARD : V + GUARD] of a V + 2 GUARD-row device allocation whose other rows hold canaries."""

    def __init__(self, init, dev, dtype=None):
        init = np.asarray(init)
        self.V = init.shape[0]
        full = np.empty((self.V + 2 * GUARD,) + init.shape[1:], init.dtype)
        canary = (np.arange(full.size, dtype=np.int64).reshape(full.shape) % 251 - 125)
        full[...] = canary.astype(init.dtype) * (3 if init.dtype.kind == "f" else 1)
        full[GUARD:self.V + GUARD] = init
        self.full = T(full, dev, dtype)
        self.view = self.full[GUARD:self.V + GUARD]
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0
        self.before = self.full.clone()

    def start(self):
        """(the values the view held when it was made, as the device holds them)"""
        return N(self.before[GUARD:self.V + GUARD])

    def intact(self, touched=None):
        """canaries, and the rows not marked in `touched` (bool [V]; None: canaries only), bit-identical to the start"""
        keep = np.ones(self.V + 2 * GUARD, bool)
        keep[GUARD:self.V + GUARD] = False if touched is None else ~np.asarray(touched, bool)
        k = torch.from_numpy(keep).to(self.full.device)
        return bool(torch.equal(_bits(self.full)[k], _bits(self.before)[k]))


def _mixed_rows(rng, n, D):
    """standard normal, a tenth of the rows scaled by 1e4 and a tenth by 1e-4: another association changes bits"""
    rows = rng.standard_normal((n, D)).astype(F32)
    s = rng.random(n)
    rows[s < 0.1] *= F32(1e4)
    rows[s > 0.9] *= F32(1e-4)
    return rows


def _scatter_runs(rng, run_idx):
    """sorted run indices -> (ids in a shuffled occurrence order over a table with unused rows, V, shuffled run indices)"""
    R = int(run_idx.max()) + 1
    V = R + R // 2 + 3
    idmap = np.sort(rng.choice(V, R, replace=False)).astype(np.int32)   # monotone: the sorted list keeps its runs
    shuffle = rng.permutation(run_idx.size)
    return idmap[run_idx][shuffle], V, run_idx[shuffle]


def _check_run_sums(dev, D, run_idx, rng, spec=None, extra=None):
    """rows_to_dense twice (fresh copies of the rows) and segment_sum_rows on a list with the runs of `run_idx`, against
    expected_run_sums bit for bit; the scratch contract of the gradient-row buffer; canaries and unused rows."""
    from esrecsys_amd import ops
    ids, V, ridx = _scatter_runs(rng, run_idx)
    R = int(run_idx.max()) + 1
    n = ids.size
    rows = _mixed_rows(rng, n, D)
    sid, perm = ops.segment_sort(T(ids, dev), V)
    s_sid = N(sid)
    assert np.array_equal(s_sid, np.sort(ids))
    if spec:
        assert_pattern(s_sid, spec)
    if extra:
        extra(s_sid)
    uniq, sums, left = expected_run_sums(ids, rows, D, scratch=True)
    exp = np.zeros((V, D), F32)
    exp[uniq] = sums
    touched = np.zeros(V, bool)
    touched[uniq] = True
    for _ in range(2):  # the second launch from fresh copies: same bits
        out = Guarded(np.full((V, D), 7.0, F32), dev)
        g = T(rows, dev)
        ops.rows_to_dense(V, D, sid, perm, g, out=out.view)
        assert same_bits(N(out.view), exp)
        assert out.intact()
        # the rows double as scratch: the first position of every chunk of a run with several chunks holds that
        # chunk's partial, every other row is unchanged
        assert same_bits(N(g), left)
    sid2, perm2 = ops.segment_sort(T(ridx, dev), R)
    g = T(rows, dev)
    assert same_bits(N(ops.segment_sum_rows(R, sid2, perm2, g)), sums)
    assert same_bits(N(g), left)
    return s_sid


# ------------------------------------------------------------------------------------------------------------------------
# 1. the run sum, bit for bit, in every instantiation
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", S1_WIDTHS)
def test_run_sum_short_runs_at_every_alignment(dev, D):
    """runs that fit the head chunk / need one continuation chunk / two, starting at positions 0, 1 and 31 mod 32"""
    spec = [(a, L) for L in SHORT_LENGTHS for a in ALIGNS]
    run_idx, _ = run_pattern(spec, tail=5)
    _check_run_sums(dev, D, run_idx, np.random.default_rng(100 + D), spec)


@pytest.mark.parametrize("D", S1_WIDTHS)
def test_run_sum_partial_counts_around_the_group_count(dev, D):
    """runs cut into NG - 1, NG, NG + 1 (the `used` clamp of the combine) and 4 NG - 1, 4 NG, 4 NG + 1, 4 NG + 3 partials
    (the exit of segment_long_kernel's four-in-flight loop), each at three alignments; the first run starts at position 0
    and the last one ends at n"""
    NG = geom(D).NG
    counts = [NG - 1, NG, NG + 1, 4 * NG - 1, 4 * NG, 4 * NG + 1, 4 * NG + 3]
    lasts = (1, CHUNK, 17)
    spec, want = [], []
    for a in ALIGNS:
        for i, P in enumerate(counts):
            spec.append((a, length_for_parts(a, P, lasts[i % 3])))
            want.append(P)
    run_idx, _ = run_pattern(spec, tail=0)

    def extra(s_sid):
        runs = runs_of(s_sid)
        have = {(p % CHUNK, n): nparts(p, n) for p, n in runs}
        assert [have[s] for s in spec] == want          # the partial counts asked for, counted on the sorted list
        assert runs[0][0] == 0 and nparts(*runs[0]) > 1  # a long run at position 0
        assert sum(runs[-1]) == s_sid.size and nparts(*runs[-1]) > 1  # a long run that ends exactly at n
    _check_run_sums(dev, D, run_idx, np.random.default_rng(200 + D), spec, extra)


@pytest.mark.parametrize("D", [64, 65, 516])
def test_run_sum_chunk_count_needs_a_second_pass(dev, D):
    """K (continuation chunks of a run) is counted 256 chunk starts per pass: runs with 255, 256 and 257 continuation
    chunks (a pass that counts exactly 256 goes round once more and counts none) and one well beyond"""
    spec = [(1, length_for_parts(1, 256, 32)), (0, length_for_parts(0, 257, 1)), (31, length_for_parts(31, 258, 5)),
            (1, 256 * CHUNK + 2 * CHUNK + 1 + 700)]
    run_idx, _ = run_pattern(spec, tail=3)

    def extra(s_sid):
        have = {(p % CHUNK, n): nparts(p, n) for p, n in runs_of(s_sid)}
        assert [have[s] - 1 for s in spec[:3]] == [255, 256, 257] and have[spec[3]] - 1 > 256 + 20
        assert spec[3][1] > 256 * CHUNK
    _check_run_sums(dev, D, run_idx, np.random.default_rng(300 + D), spec, extra)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65])
def test_run_sum_whole_list_is_one_run(dev, n):
    """one run of n positions (the long launch is issued only for n > 32; its boundary count is (n - 1) / 32), every width"""
    for D in S1_WIDTHS:
        run_idx = np.zeros(n, np.int32)
        s_sid = _check_run_sums(dev, D, run_idx, np.random.default_rng(n * 2000 + D))
        assert runs_of(s_sid) == [(0, n)]


@pytest.mark.parametrize("D", [260, 130])
def test_run_sum_beyond_the_grid_cap(dev, D):
    """more than 2048 * NG positions at G = 64: the grid is capped, every row group walks a slice of several positions and
    slices begin inside runs (short and long ones mixed)"""
    g = geom(D)
    assert g.G == 64 and g.NG == 4
    rng = np.random.default_rng(400 + D)
    spec, total = [], 0
    while total < 3 * MAX_GRID * g.NG:
        L = int(rng.choice([1, 1, 2, 3, 5, 17, 33, 40, 64, 70, 97, 130, 300, 1100]))
        spec.append((int(rng.integers(0, CHUNK)), L))
        total += L
    run_idx, _ = run_pattern(spec, tail=1)

    def extra(s_sid):
        n = s_sid.size
        ngroups = MAX_GRID * g.NG
        assert n > 2 * ngroups
        per = -(-n // ngroups)
        starts = np.arange(per, n, per)
        inside = s_sid[starts] == s_sid[starts - 1]
        assert per >= 3 and inside.sum() > 100 and (~inside).sum() > 100
    _check_run_sums(dev, D, run_idx, rng, None, extra)


def _small_list(D, seed=0):
    rng = np.random.default_rng(seed + D)
    V, n = 6, 40   # ~7 occurrences per row, and one row never named
    ids = rng.integers(0, V - 1, n).astype(np.int32)
    rows = (rng.standard_normal((n, D)) * 0.1).astype(F32)
    return rng, V, n, ids, rows


@pytest.mark.parametrize("D", REFUSED)
def test_refused_widths_touch_nothing(dev, D):
    """more than four chunks per lane: every entry point raises the library's "not supported" and leaves table,
    accumulator and canaries as they were (rows_to_dense zero-fills its output before the check)"""
    from esrecsys_amd import ops
    from esrecsys_amd._lib import EsrLibraryError
    assert geom(D).NCH is None
    rng, V, n, ids, rows = _small_list(D)
    sid, perm = ops.segment_sort(T(ids, dev), V)
    p0 = rng.standard_normal((V, D)).astype(F32)
    a0 = (0.1 + rng.random((V, D))).astype(F32)
    none = np.zeros(V, bool)
    out = Guarded(np.full((V, D), 7.0, F32), dev)
    with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
        ops.rows_to_dense(V, D, sid, perm, T(rows, dev), out=out.view)
    assert out.intact() and not N(out.view).any()
    with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
        ops.segment_sum_rows(V - 1, sid, perm, T(rows, dev))
    for dtype in (None, torch.bfloat16):
        table, accum = Guarded(p0, dev, dtype), Guarded(a0, dev)
        with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
            ops.sparse_adagrad(table.view, accum.view, sid, perm, T(rows, dev), 0.05, 1e-7)
        with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
            ops.sparse_sgd(table.view, sid, perm, T(rows, dev), 0.01)
        with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
            ops.sparse_adagrad_multi([table.view], [accum.view], [0, V], sid, perm, T(rows, dev), 0.05, 1e-7)
        assert table.intact(none) and accum.intact(none)
    table, trace, nu = Guarded(p0, dev), Guarded(a0, dev), Guarded(a0, dev)
    last = Guarded(np.full(V, 11, np.int32), dev)
    with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
        ops.sparse_momentum(table.view, trace.view, sid, perm, T(rows, dev), 0.01)
    with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
        ops.sparse_momentum_step(table.view, trace.view, sid, perm, T(rows, dev), 0.01, 0.9)
    with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
        ops.sparse_momentum_step_multi([table.view], [trace.view], [0, V], sid, perm, T(rows, dev), 0.01, 0.9)
    with pytest.raises(EsrLibraryError, match="D=%d not supported" % D):
        ops.sparse_adam_step_lazy([table.view], [trace.view], [nu.view], [last.view], [0, V], sid, perm, T(rows, dev),
                                  1e-3, 12)
    assert table.intact(none) and trace.intact(none) and nu.intact(none) and last.intact(none)


# ------------------------------------------------------------------------------------------------------------------------
# 2. every op on every instantiation, against float64
# ------------------------------------------------------------------------------------------------------------------------
def _pattern_spec(D):
    NG = geom(D).NG
    spec = [(a, L) for L in SHORT_LENGTHS for a in ALIGNS]
    if NG <= 16:  # (wider row groups: section 1 holds those counts; here the list stays a few thousand positions)
        spec += [(1, length_for_parts(1, NG + 1, 9)), (31, length_for_parts(31, 4 * NG + 1, 32))]
    return spec


@functools.lru_cache(maxsize=None)
def _case(D, kind):
    """ids / gradient rows / start values of one (width, id kind), with the float64 and the float32 run sums.  Shared by
    the tests of section 2 (read only)."""
    rng = np.random.default_rng(7000 + 10 * D + KINDS.index(kind))
    V, n = 400, 1500
    spec = None
    if kind == "uniform":
        ids = rng.integers(0, V, n).astype(np.int32)
    elif kind == "same":
        ids = np.full(n, V - 1, np.int32)   # (bf16 bars: at most ~5000 occurrences of one row, see the module docstring)
    elif kind == "zipf":
        p = 1.0 / np.arange(1, V + 1)
        ids = rng.permutation(V)[rng.choice(V, size=n, p=p / p.sum())].astype(np.int32)
    else:
        spec = _pattern_spec(D)
        run_idx, _ = run_pattern(spec, tail=2)
        ids, V, _ = _scatter_runs(rng, run_idx)
        n = ids.size
    rows = (rng.standard_normal((n, D)) * 0.1).astype(F32)
    G = np.zeros((V, D), F64)
    np.add.at(G, ids, rows.astype(F64))
    uniq, g32 = expected_run_sums(ids, rows, D)
    touched = np.zeros(V, bool)
    touched[uniq] = True
    assert not touched.all() or kind == "zipf"
    c = dict(V=V, n=n, ids=ids, rows=rows, G=G, uniq=uniq, g32=g32, touched=touched, spec=spec,
             p0=rng.standard_normal((V, D)).astype(F32), a0=(0.1 + rng.random((V, D))).astype(F32),
             t0=(rng.standard_normal((V, D)) * 0.3).astype(F32))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _sorted(dev, c):
    from esrecsys_amd import ops
    sid, perm = ops.segment_sort(T(c["ids"], dev), c["V"])
    if c["spec"]:
        assert_pattern(N(sid), c["spec"])
    return sid, perm


def _trunc_bf16(x):
    """x cut to bf16's 8 significant bits TOWARDS ZERO: what a store that drops the low half of the f32 word leaves"""
    m, e = np.frexp(np.asarray(x, F64))
    return np.ldexp(np.trunc(m * 256.0) / 256.0, e)


def _bf16_close(got, exp64, touched):
    """The bf16 bars of test_sparse_adagrad_bf16_table -- rel_err <= 2^-8, share of elements equal to RNE(float64) above
    0.999 -- over the whole tables as there AND over the touched rows alone (below 1000 touched elements that reads: no
    element off).  got / exp64 / touched: lists, one entry per table the list was applied to (_bf16_tables).  The touched
    elements must be able to tell a store that rounds from one that truncates: some of them round UP."""
    for g, e in zip(got, exp64):
        assert rel_err(g, e) <= 2.0 ** -8
        assert np.mean(g == o_optim.round_bf16(e)) > 0.999
    g = np.concatenate([x[t].ravel() for x, t in zip(got, touched)])
    e = np.concatenate([x[t].ravel() for x, t in zip(exp64, touched)])
    assert rel_err(g, e) <= 2.0 ** -8
    rne = o_optim.round_bf16(e)
    off = int(np.count_nonzero(g != rne))
    share = 1.0 - off / g.size
    print("bf16 share of touched elements equal to RNE(float64): %.6f (%d of %d off)" % (share, off, g.size))
    assert share > 0.999
    assert g.size >= 64 and np.count_nonzero(rne != _trunc_bf16(e)) >= 8


def _start_tables(c, dtype):
    """The start tables one list is applied to: c["p0"], and for a bf16 table whose touched rows hold fewer than 64
    elements (`same` at D = 1 and D = 3: one row) as many further tables as it takes to see 64 touched elements -- one
    element, or three, could not tell a rounding store from a truncating one."""
    tables = [c["p0"]]
    if dtype == torch.bfloat16:
        per = int(c["touched"].sum()) * c["p0"].shape[1]
        rng = np.random.default_rng(per)
        while per * len(tables) < 64:
            tables.append(rng.standard_normal(c["p0"].shape).astype(F32))
    return tables


S2 = pytest.mark.parametrize("D,kind", [(D, k) for D in S2_WIDTHS for k in KINDS])
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


@DTYPES
@S2
def test_adagrad_every_width(dev, D, kind, dtype):
    from esrecsys_amd import ops
    c = _case(D, kind)
    sid, perm = _sorted(dev, c)
    got, exp = [], []
    for p0 in _start_tables(c, dtype):
        table, accum = Guarded(p0, dev, dtype), Guarded(c["a0"], dev)
        ops.sparse_adagrad(table.view, accum.view, sid, perm, T(c["rows"], dev), 0.05, 1e-7)
        ep, ea = o_optim.sparse_adagrad_update(table.start().astype(F64), c["a0"].astype(F64), c["ids"],
                                               c["rows"].astype(F64), 0.05, 1e-7, F64)
        assert table.intact(c["touched"]) and accum.intact(c["touched"])
        assert rel_err(N(accum.view), ea) <= TOL
        got.append(N(table.view)), exp.append(ep)
    if dtype == torch.float32:
        assert rel_err(got[0], exp[0]) <= TOL
    else:
        _bf16_close(got, exp, [c["touched"]] * len(got))


@DTYPES
@S2
def test_sgd_every_width(dev, D, kind, dtype):
    from esrecsys_amd import ops
    c = _case(D, kind)
    sid, perm = _sorted(dev, c)
    got, exp = [], []
    for p0 in _start_tables(c, dtype):
        table = Guarded(p0, dev, dtype)
        ops.sparse_sgd(table.view, sid, perm, T(c["rows"], dev), 0.01)
        assert table.intact(c["touched"])
        got.append(N(table.view)), exp.append(table.start().astype(F64) - 0.01 * c["G"])
    if dtype == torch.float32:
        assert rel_err(got[0], exp[0]) <= TOL
    else:
        _bf16_close(got, exp, [c["touched"]] * len(got))


@S2
def test_momentum_gradient_half_every_width(dev, D, kind):
    """ops.sparse_momentum (kMomentum): trace += G ; p -= lr * G on the touched rows"""
    from esrecsys_amd import ops
    c = _case(D, kind)
    table, trace = Guarded(c["p0"], dev), Guarded(c["t0"], dev)
    sid, perm = _sorted(dev, c)
    ops.sparse_momentum(table.view, trace.view, sid, perm, T(c["rows"], dev), 0.01)
    assert table.intact(c["touched"]) and trace.intact(c["touched"])
    assert rel_err(N(trace.view), c["t0"].astype(F64) + c["G"]) <= TOL
    assert rel_err(N(table.view), c["p0"].astype(F64) - 0.01 * c["G"]) <= TOL


@pytest.mark.parametrize("numel", [1, 3, 4, 4003, 400 * 130])
def test_momentum_decay_half(dev, numel):
    """ops.dense_momentum_decay: trace *= m ; p -= lr * trace over float4 chunks and the scalar tail"""
    from esrecsys_amd import ops
    rng = np.random.default_rng(numel)
    p0, t0 = rng.standard_normal(numel).astype(F32), rng.standard_normal(numel).astype(F32)
    p, tr = Guarded(p0, dev), Guarded(t0, dev)
    ops.dense_momentum_decay(p.view, tr.view, 0.01, 0.9)
    assert p.intact() and tr.intact()
    et = t0.astype(F64) * 0.9
    assert rel_err(N(tr.view), et) <= TOL and rel_err(N(p.view), p0.astype(F64) - 0.01 * et) <= TOL


@S2
def test_momentum_both_halves_are_one_optax_step(dev, D, kind):
    """decay half over the whole table, then the gradient half on the touched rows == optax.sgd(lr, momentum)"""
    from esrecsys_amd import ops
    c = _case(D, kind)
    table, trace = Guarded(c["p0"], dev), Guarded(c["t0"], dev)
    sid, perm = _sorted(dev, c)
    ops.dense_momentum_decay(table.view, trace.view, 0.01, 0.9)
    ops.sparse_momentum(table.view, trace.view, sid, perm, T(c["rows"], dev), 0.01)
    ep, et = o_spotify.sgd_momentum_update(c["p0"].astype(F64), c["t0"].astype(F64), c["G"], 0.01, 0.9, F64)
    assert table.intact() and trace.intact()
    assert rel_err(N(table.view), ep) <= TOL and rel_err(N(trace.view), et) <= TOL


@S2
def test_momentum_step_every_width_bit_exact(dev, D, kind):
    """ops.sparse_momentum_step (kMomentumStep): tr = g + m * tr ; p = p - lr * tr with every operation rounded on its
    own (the kernel spells them __f*_rn), g the run sum in the kernels' order: float32 numpy gives the same bits"""
    from esrecsys_amd import ops
    c = _case(D, kind)
    table, trace = Guarded(c["p0"], dev), Guarded(c["t0"], dev)
    sid, perm = _sorted(dev, c)
    ops.sparse_momentum_step(table.view, trace.view, sid, perm, T(c["rows"], dev), 0.01, 0.9)
    u = c["uniq"]
    tr = c["g32"] + F32(0.9) * c["t0"][u]
    p = c["p0"][u] - F32(0.01) * tr
    assert tr.dtype == F32 and p.dtype == F32
    assert table.intact(c["touched"]) and trace.intact(c["touched"])
    assert same_bits(N(trace.view)[u], tr) and same_bits(N(table.view)[u], p)
    ep, et = o_optim.sgd_momentum_update(c["p0"][u].astype(F64), c["t0"][u].astype(F64), c["G"][u], 0.01, 0.9, F64)
    assert rel_err(N(table.view)[u], ep) <= TOL and rel_err(N(trace.view)[u], et) <= TOL


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [3, 65, 130, 255, 260, 516, 1024])
def test_lazy_adam_step_equals_dense_adam_every_width(dev, D, kind):
    """one lazy step on rows with last = step - 1 against rows_to_dense + dense_adam on the same list, bit for bit on the
    touched rows; V is odd, so at the odd widths V * D is no multiple of 4 and the last elements of the table take the
    dense kernel's scalar-tail form (adam_is_tail)"""
    from esrecsys_amd import ops
    c = _case(D, kind)
    step, lr = 12, 1e-3
    V = c["V"] + 1 - c["V"] % 2   # an odd table (the list never names the added row)
    rng = np.random.default_rng(D)
    pad = lambda a: np.concatenate([a, a[:V - a.shape[0]]])  # noqa: E731
    touched = pad(c["touched"]).copy()
    touched[c["V"]:] = False
    assert V % 2 == 1 and ((V * D) % 4 != 0) == (D % 4 != 0)
    rows = (c["rows"] * F32(0.1))
    tabs = [Guarded(pad(c["p0"]), dev), Guarded(pad(c["t0"]) * F32(0.01), dev),
            Guarded((rng.random((V, D)) * 1e-4).astype(F32), dev)]
    last = Guarded(np.full(V, step - 1, np.int32), dev)
    sid, perm = ops.segment_sort(T(c["ids"], dev), V)
    dense = [t.view.clone() for t in tabs]
    g_all = ops.rows_to_dense(V, D, sid, perm, T(rows, dev))
    ops.dense_adam(dense[0], dense[1], dense[2], g_all, lr, step)
    ops.sparse_adam_step_lazy([tabs[0].view], [tabs[1].view], [tabs[2].view], [last.view], [0, V], sid, perm, T(rows, dev),
                              lr, step)
    assert last.intact(touched) and (N(last.view)[touched] == step).all()
    for t, d in zip(tabs, dense):
        assert t.intact(touched)
        assert same_bits(N(t.view)[touched], N(d)[touched])
    assert not same_bits(N(tabs[0].view)[touched], tabs[0].start()[touched])


def test_lazy_adam_tail_elements_carry_a_gradient(dev):
    """D = 3, V = 5 (V * D = 15: the last three elements, the whole last row, are the dense kernel's scalar tail) with the
    last row in the list"""
    from esrecsys_amd import ops
    D, V, step, lr = 3, 5, 12, 1e-3
    rng = np.random.default_rng(5)
    ids = np.array([4, 0, 4, 2, 4, 3, 3], np.int32)
    rows = (rng.standard_normal((ids.size, D)) * 0.01).astype(F32)
    touched = np.array([1, 0, 1, 1, 1], bool)
    tabs = [Guarded(rng.standard_normal((V, D)).astype(F32), dev), Guarded((rng.standard_normal((V, D)) * 1e-3).astype(F32), dev),
            Guarded((rng.random((V, D)) * 1e-4).astype(F32), dev)]
    last = Guarded(np.full(V, step - 1, np.int32), dev)
    sid, perm = ops.segment_sort(T(ids, dev), V)
    dense = [t.view.clone() for t in tabs]
    ops.dense_adam(dense[0], dense[1], dense[2], ops.rows_to_dense(V, D, sid, perm, T(rows, dev)), lr, step)
    ops.sparse_adam_step_lazy([tabs[0].view], [tabs[1].view], [tabs[2].view], [last.view], [0, V], sid, perm, T(rows, dev),
                              lr, step)
    for t, d in zip(tabs, dense):
        assert t.intact(touched) and same_bits(N(t.view)[touched], N(d)[touched])
    assert last.intact(touched) and (N(last.view)[touched] == step).all()


# ------------------------------------------------------------------------------------------------------------------------
# 3. fused tables
# ------------------------------------------------------------------------------------------------------------------------
FUSED_V = (37, 53, 41, 29)
FUSED_GAP = (3, 0, 7, 5)   # padded row offsets; none between tables 1 and 2: their edge rows are ADJACENT virtual ids


def _fused_case(D, nt, seed):
    rng = np.random.default_rng(seed + D + nt)
    Vt = FUSED_V[:nt]
    offs = [0]
    for k in range(nt):
        offs.append(offs[-1] + Vt[k] + FUSED_GAP[k])
    lists = []
    for k in range(nt):
        i = rng.integers(0, Vt[k], 260).astype(np.int32)
        i[:70] = Vt[k] - 1          # a hot row at the last row of every table ...
        i[70:140] = 0               # ... and at row 0 of the next one: neighbours in the sorted list, not one run
        lists.append(rng.permutation(i))
    rows = [(rng.standard_normal((l.size, D)) * 0.1).astype(F32) for l in lists]
    p0 = [rng.standard_normal((V, D)).astype(F32) for V in Vt]
    a0 = [(0.1 + rng.random((V, D))).astype(F32) for V in Vt]
    vids = np.concatenate([l + offs[k] for k, l in enumerate(lists)]).astype(np.int32)
    return Vt, offs, lists, rows, p0, a0, vids


def _one_chunk_rows(sorted_ids, V, base=0):
    """bool [V]: rows whose run is a single chunk at its position in this sorted list (rows without a run: True)"""
    ok = np.ones(V, bool)
    s = np.asarray(sorted_ids)
    for p, n in runs_of(s):
        ok[int(s[p]) - base] = nparts(p, n) == 1
    return ok


@pytest.mark.parametrize("op", ["adagrad", "momentum_step"])
@pytest.mark.parametrize("nt", [1, 2, 3, 4])
@pytest.mark.parametrize("D", [130, 516])
def test_fused_tables_equal_per_table_calls(dev, D, nt, op):
    """one sort + one launch pair over 1 .. 4 tables addressed by virtual rows == the per-table calls on the per-table lists
    (bit for bit on rows whose occurrences sit in one chunk in both layouts, TOL elsewhere) == float64"""
    from esrecsys_amd import ops
    Vt, offs, lists, rows, p0, a0, vids = _fused_case(D, nt, 31)
    sv, perm = ops.segment_sort(T(vids, dev), offs[-1])
    s_sv = N(sv)
    for k in range(nt - 1):   # the edge rows of neighbouring tables are separate runs
        hi, lo = offs[k] + Vt[k] - 1, offs[k + 1]
        assert np.count_nonzero(s_sv == hi) >= 70 and np.count_nonzero(s_sv == lo) >= 70
        assert s_sv[np.flatnonzero(s_sv == hi)[-1] + 1] == lo
    ft, fa = [Guarded(p, dev) for p in p0], [Guarded(a, dev) for a in a0]
    all_rows = T(np.concatenate(rows), dev)
    if op == "adagrad":
        ops.sparse_adagrad_multi([t.view for t in ft], [a.view for a in fa], offs, sv, perm, all_rows, 0.05, 1e-7)
    else:
        ops.sparse_momentum_step_multi([t.view for t in ft], [a.view for a in fa], offs, sv, perm, all_rows, 0.01, 0.9)
    for k in range(nt):
        pt, pa = Guarded(p0[k], dev), Guarded(a0[k], dev)
        s, q = ops.segment_sort(T(lists[k], dev), Vt[k])
        G = np.zeros((Vt[k], D), F64)
        np.add.at(G, lists[k], rows[k].astype(F64))
        if op == "adagrad":
            ops.sparse_adagrad(pt.view, pa.view, s, q, T(rows[k], dev), 0.05, 1e-7)
            ep, ea = o_optim.sparse_adagrad_update(p0[k].astype(F64), a0[k].astype(F64), lists[k], rows[k].astype(F64),
                                                   0.05, 1e-7, F64)
        else:
            ops.sparse_momentum_step(pt.view, pa.view, s, q, T(rows[k], dev), 0.01, 0.9)
            u = np.unique(lists[k])
            ep, ea = p0[k].astype(F64), a0[k].astype(F64)
            ep[u], ea[u] = o_optim.sgd_momentum_update(ep[u], ea[u], G[u], 0.01, 0.9, F64)
        touched = np.zeros(Vt[k], bool)
        touched[lists[k]] = True
        assert ft[k].intact(touched) and fa[k].intact(touched) and pt.intact(touched) and pa.intact(touched)
        one = _one_chunk_rows(N(s), Vt[k]) & _one_chunk_rows(s_sv[(s_sv >= offs[k]) & (s_sv < offs[k + 1])], Vt[k], offs[k])
        in_fused = {int(s_sv[p]): nparts(p, n) == 1 for p, n in runs_of(s_sv)}
        one &= np.array([in_fused.get(offs[k] + r, True) for r in range(Vt[k])])
        assert one.sum() > Vt[k] - 3 and (nt == 1 or not one.all())
        assert same_bits(N(ft[k].view)[one], N(pt.view)[one]) and same_bits(N(fa[k].view)[one], N(pa.view)[one])
        assert rel_err(N(ft[k].view), N(pt.view)) <= TOL and rel_err(N(fa[k].view), N(pa.view)) <= TOL
        assert rel_err(N(ft[k].view), ep) <= TOL and rel_err(N(fa[k].view), ea) <= TOL


@pytest.mark.parametrize("op", ["adagrad", "momentum_step"])
def test_five_fused_tables_are_refused(dev, op):
    from esrecsys_amd import ops
    from esrecsys_amd._lib import EsrLibraryError
    D, V = 130, 9
    rng = np.random.default_rng(3)
    tabs = [Guarded(rng.standard_normal((V, D)).astype(F32), dev) for _ in range(5)]
    accs = [Guarded((0.1 + rng.random((V, D))).astype(F32), dev) for _ in range(5)]
    offs = [V * k for k in range(6)]
    vids = rng.integers(0, 5 * V, 64).astype(np.int32)
    sv, perm = ops.segment_sort(T(vids, dev), 5 * V)
    rows = T((rng.standard_normal((64, D)) * 0.1).astype(F32), dev)
    with pytest.raises(EsrLibraryError, match=r"ntables=5 not in \[1, 4\]"):
        if op == "adagrad":
            ops.sparse_adagrad_multi([t.view for t in tabs], [a.view for a in accs], offs, sv, perm, rows, 0.05, 1e-7)
        else:
            ops.sparse_momentum_step_multi([t.view for t in tabs], [a.view for a in accs], offs, sv, perm, rows, 0.01, 0.9)
    none = np.zeros(V, bool)
    assert all(t.intact(none) for t in tabs) and all(a.intact(none) for a in accs)


@pytest.mark.parametrize("D", [130, 516])
def test_fused_long_runs_hint_off_equals_default(dev, D):
    """long_runs = 0 (the caller knows no run outgrows its head chunk: the long launch is skipped) == long_runs = -1, bit
    for bit, on such a list"""
    from esrecsys_amd import ops
    rng = np.random.default_rng(D)
    Vt, offs = (300, 200, 250), [0, 304, 504, 760]
    lists = [rng.integers(0, V, 500).astype(np.int32) for V in Vt]
    for l in lists:
        l[:30] = 7   # a run of 30-odd: fits any head chunk
    vids = np.concatenate([l + offs[k] for k, l in enumerate(lists)]).astype(np.int32)
    rows = (rng.standard_normal((vids.size, D)) * 0.1).astype(F32)
    sv, perm = ops.segment_sort(T(vids, dev), offs[-1])
    runs = runs_of(N(sv))
    assert all(nparts(p, n) == 1 for p, n in runs) and max(n for _, n in runs) >= 30
    p0 = [rng.standard_normal((V, D)).astype(F32) for V in Vt]
    res = []
    for hint in (-1, 0):
        ft, fa = [Guarded(p, dev) for p in p0], [Guarded(np.full(p.shape, 0.1, F32), dev) for p in p0]
        ops.sparse_adagrad_multi([t.view for t in ft], [a.view for a in fa], offs, sv, perm, T(rows, dev), 0.05, 1e-7,
                                 long_runs=hint)
        assert all(t.intact() for t in ft + fa)
        res.append([N(t.view) for t in ft + fa])
    assert all(same_bits(a, b) for a, b in zip(*res))
    assert not same_bits(res[0][0], p0[0])


# ------------------------------------------------------------------------------------------------------------------------
# 4. two argument checks
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("D", [8, 6, 260, 512])  # (6: no vector lanes at all; 260, 512: more chunks than one wave has lanes)
def test_rows_consolidate_on_a_view_offset_by_one_element(dev, D, dtype):
    """a [V, D] view that starts one element into its allocation (2-byte aligned bf16, 4-byte aligned f32) cannot take the
    8 / 16-byte lanes: the call copies element-wise and gives what it gives on aligned buffers"""
    from esrecsys_amd import ops
    rng = np.random.default_rng(D)
    V = 70
    prim = T(rng.standard_normal((V, D)).astype(F32), dev, dtype)
    shad = T(rng.standard_normal((V, D)).astype(F32), dev, dtype)
    loc0 = rng.choice(np.array([0, 1, 2, 3, 7], np.uint8), V)
    a_p, a_loc = prim.clone(), T(loc0, dev)
    ops.rows_consolidate(a_p, shad.clone(), a_loc)
    moved = (loc0 & 1).astype(bool)
    assert same_bits(N(a_p)[moved], N(shad)[moved]) and same_bits(N(a_p)[~moved], N(prim)[~moved]) and not N(a_loc).any()

    def offset_view(t):
        flat = torch.full((V * D + 2,), 99.0, dtype=dtype, device=dev)
        flat[1:V * D + 1] = t.reshape(-1)
        v = flat[1:V * D + 1].view(V, D)
        assert v.is_contiguous() and v.data_ptr() % (4 * t.element_size()) != 0
        return flat, v
    fp, vp = offset_view(prim)
    fs, vs = offset_view(shad)
    loc = T(loc0, dev)
    ops.rows_consolidate(vp, vs, loc)
    assert same_bits(N(vp), N(a_p)) and not N(loc).any()
    assert float(fp[0]) == 99.0 and float(fp[-1]) == 99.0 and same_bits(N(vs), N(shad))


def test_pass_c_forms_must_hold_eight_words(dev):
    """the library copies 8 int32 into pass_c_forms: a shorter or strided tensor is refused before anything is launched"""
    from esrecsys_amd import ops
    B, D = 128, 128
    g = torch.Generator().manual_seed(0)
    Q, C = (torch.randn((B, D), generator=g) * 0.1).to(dev), (torch.randn((B, D), generator=g) * 0.1).to(dev)
    with pytest.raises(ValueError, match="at least 8"):
        ops.inbatch_softmax_fwd_bwd(Q, C, 1.0, 0.0, float(B), precision="f16x2",
                                    pass_c_forms=torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        ops.inbatch_softmax_fwd_bwd(Q, C, 1.0, 0.0, float(B), precision="f16x2",
                                    pass_c_forms=torch.zeros(16, dtype=torch.int32, device=dev)[::2])
    forms = torch.full((8,), -5, dtype=torch.int32, device=dev)
    ops.inbatch_softmax_fwd_bwd(Q, C, 1.0, 0.0, float(B), precision="f16x2", pass_c_forms=forms)
    assert (N(forms) != -5).all()

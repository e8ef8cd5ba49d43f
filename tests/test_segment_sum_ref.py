"""CPU: the tests' own restatement of the row-sparse update engine (tests/_segment_sum_ref.py) -- the geometry table the
GPU tests of tests/test_gpu_segment_update.py name their cases by, pinned against the constants of the source, and the
run-pattern / summation-order helpers against plain definitions."""
import os
import re

import numpy as np
import pytest

from _segment_sum_ref import (BLOCK, CHUNK, MAX_GRID, MAX_NCH, WAVE, assert_pattern, chunk_bounds, expected_run_sums, geom,
                              length_for_parts, nparts, run_pattern, runs_of)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esrecsys_amd", "csrc")

# D: (VEC, lanes per row G, chunks per lane nch, template NCH, row groups per workgroup NG)
GEOMETRY = {
    1: (1, 1, 1, 1, 256), 2: (1, 2, 1, 1, 128), 3: (1, 4, 1, 1, 64), 4: (4, 1, 1, 1, 256), 8: (4, 2, 1, 1, 128),
    63: (1, 64, 1, 1, 4), 64: (4, 16, 1, 1, 16), 65: (1, 64, 2, 2, 4), 100: (4, 32, 1, 1, 8), 127: (1, 64, 2, 2, 4),
    130: (1, 64, 3, 4, 4), 192: (4, 64, 1, 1, 4), 193: (1, 64, 4, 4, 4), 255: (1, 64, 4, 4, 4), 256: (4, 64, 1, 1, 4),
    260: (4, 64, 2, 2, 4), 512: (4, 64, 2, 2, 4), 516: (4, 64, 3, 4, 4), 768: (4, 64, 3, 4, 4), 772: (4, 64, 4, 4, 4),
    1024: (4, 64, 4, 4, 4),
}


def test_geometry_table_of_the_segment_update_tests():
    """every width section 1 of the GPU module runs, against the dispatch table written out by hand; the refused widths"""
    for D, (vec, G, nch, NCH, NG) in GEOMETRY.items():
        g = geom(D)
        assert (g.vec, g.G, g.nch, g.NCH, g.NG) == (vec, G, nch, NCH, NG), D
        assert g.nvec * g.vec == D and g.G * g.NG == BLOCK and (g.nch - 1) * g.G < g.nvec <= g.nch * g.G
    for D in (257, 258, 1028, 1025, 2048):
        assert geom(D).NCH is None and geom(D).nch > MAX_NCH
    # all six <VEC, NCH> instantiations occur
    assert {(v[0], v[3]) for v in GEOMETRY.values()} == {(1, 1), (1, 2), (1, 4), (4, 1), (4, 2), (4, 4)}


def test_geometry_constants_are_the_sources():
    """the constants geom() and the chunk plan are built on, read from the headers: a change there makes this table stale"""
    common = open(os.path.join(CSRC, "esr_common.h")).read()
    segment = open(os.path.join(CSRC, "esr_segment.h")).read()

    def const(text, name):
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
        assert m, name
        return int(eval(m.group(1), {"__builtins__": {}}))  # "256 * 8"
    assert const(common, "kBlock") == BLOCK and const(common, "kWave") == WAVE
    assert const(common, "kMaxChunksPerLane") == MAX_NCH and const(common, "kMaxGrid") == MAX_GRID
    assert const(segment, "kSegChunk") == CHUNK and const(segment, "kMaxFusedTables") == 4
    # row_geom's rule and the dispatch's cut points, as text
    assert "g.vec = (D % 4 == 0) ? 4 : 1;" in common and "while (G < g.nvec && G < kWave) G <<= 1;" in common
    assert re.search(r"\(geom\)\.nch <= 1\).*NCH = 1;.*\n.*\(geom\)\.nch <= 2\).*NCH = 2;.*\n.*NCH = 4;", common)


@pytest.mark.parametrize("align", [0, 1, 17, 31])
def test_chunk_plan(align):
    for length in (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 500):
        b = chunk_bounds(align, align + length)
        assert b[0][0] == align and b[-1][1] == align + length and all(x[1] == y[0] for x, y in zip(b, b[1:]))
        assert all(c % CHUNK == 0 and e - c <= CHUNK for c, e in b[1:])
        head = b[0][1] - b[0][0]
        assert head <= 2 * CHUNK - 1 and (len(b) == 1 or (head >= CHUNK and b[0][1] % CHUNK == 0))
    for parts in (2, 3, 4, 5, 17, 1027):
        for last in (1, 17, CHUNK):
            assert nparts(align, length_for_parts(align, parts, last)) == parts
        assert nparts(align, length_for_parts(align, parts, 1) - 1) == parts - 1


def test_run_pattern_puts_runs_where_asked():
    spec = [(a, L) for L in (1, 33, 64, 97) for a in (0, 1, 31)]
    idx, named = run_pattern(spec, tail=4)
    assert np.array_equal(idx, np.sort(idx)) and len(named) == len(spec)
    runs = dict((int(idx[p]), (p % CHUNK, n)) for p, n in runs_of(idx))
    assert [runs[r] for r in named] == spec
    assert_pattern(idx, spec)
    with pytest.raises(AssertionError):
        assert_pattern(idx, [(5, 97)])
    assert runs_of(idx)[-1][1] == 1 and runs_of(np.zeros(0, np.int32)) == []


@pytest.mark.parametrize("D", [1, 3, 32, 130, 516])
def test_expected_run_sums_against_plain_definitions(D):
    """close to the float64 sum everywhere; equal to the sequential float32 sum where a run is one chunk; the chunked order
    written out naively for the others; the scratch buffer holds the chunk partials"""
    rng = np.random.default_rng(D)
    NG = geom(D).NG
    spec = [(0, 5), (1, 63), (31, 33), (0, 32), (31, 34), (1, 64), (0, length_for_parts(0, NG + 2, 3))]
    idx, named = run_pattern(spec, tail=2)
    shuffle = rng.permutation(idx.size)
    ids, rows = idx[shuffle], rng.standard_normal((idx.size, D)).astype(np.float32)
    uniq, sums, left = expected_run_sums(ids, rows, D, scratch=True)
    assert np.array_equal(uniq, np.arange(idx.max() + 1))
    G = np.zeros((uniq.size, D))
    np.add.at(G, ids, rows.astype(np.float64))
    assert np.max(np.abs(sums - G)) <= 1e-6 * np.max(np.abs(G))
    order = np.argsort(ids, kind="stable")
    changed = np.zeros(idx.size, bool)
    for p, n in runs_of(ids[order]):
        b = chunk_bounds(p, p + n)
        parts = []
        for c, e in b:
            acc = rows[order[c]].copy()
            for k in range(c + 1, e):
                acc = acc + rows[order[k]]
            parts.append(acc)
        if len(b) == 1:
            total = parts[0]
        else:
            gs = []
            for g in range(min(NG, len(parts))):
                acc = np.zeros(D, np.float32)
                for i in range(g, len(parts), NG):
                    acc = acc + parts[i]
                gs.append(acc)
            total = gs[0]
            for g in gs[1:]:
                total = total + g
            for (c, _), part in zip(b, parts):
                changed[order[c]] = True
                assert np.array_equal(left[order[c]], part)
        assert np.array_equal(sums[ids[order[p]]], total)
    assert np.array_equal(left[~changed], rows[~changed]) and changed.sum() >= NG + 2 + 2 + 2

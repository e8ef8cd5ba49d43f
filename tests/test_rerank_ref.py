"""CPU: the NumPy restatement of the re-ranking rule (tests/_rerank_ref.py) -- hand-worked lists, lam = 1 as the stable sort,
ties, the exact tables exact in fp64 (and their similarities equal to a plain fp64 matrix product), the fp64 order witnesses
of the intra-list similarity, and esr_rerank_rule.h (the text the kernels compile) against the restatement through a
stand-alone host program built plain and with the address and undefined-behaviour sanitizers
(tests/host/rerank_rule_host.cpp; no HIP, not loaded into Python)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _rerank_ref as rref
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _unit(*rows):
    return np.array(rows, np.float32)


# ---- hand-worked lists -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mmr_demotes_a_near_duplicate(dtype):
    """three items: A and its copy A' (sim 1) score 1 and 0.75, B (orthogonal to both) scores 0.5.  By score: A, A', B.  At
    lam = 0.5 round 1 values A' at 0.5 * 0.75 - 0.5 * 1 = -0.125 and B at 0.25 - 0 = 0.25: B overtakes the copy."""
    rows = _unit([1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0])
    cand, rel = np.array([0, 1, 2]), np.array([1.0, 0.75, 0.5], np.float32)
    r = rref.mmr_query(rows, cand, rel, 3, 0.5, 3, dtype)
    assert r["pos"].tolist() == [0, 2, 1] and r["length"] == 3 and r["failed"] == 0
    assert r["value"].tolist() == [0.5, 0.25, -0.125] and r["rel"].tolist() == [1.0, 0.5, 0.75]
    assert rref.mmr_query(rows, cand, rel, 3, 1.0, 3, dtype)["pos"].tolist() == [0, 1, 2]
    # lam = 0: relevance is ignored; round 0 is a tie of zeros (position 0), then the least similar
    assert rref.mmr_query(rows, cand, rel, 3, 0.0, 3, dtype)["pos"].tolist() == [0, 2, 1]
    # m is the GREATEST similarity to the picks so far: after A and B the copy is still held back by A
    assert rref.mmr_query(rows, cand, rel, 3, 0.5, 3, dtype)["values"][2][1] == -0.125


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lam_one_is_the_stable_sort_and_ties_go_to_the_lower_position(dtype):
    rng = np.random.default_rng(0)
    rows = rref.exact_table(rng, 40, 8)
    cand = rng.integers(0, 40, 30)
    rel = rng.integers(-3, 4, 30).astype(np.float32) / 2                      # many ties
    r = rref.mmr_query(rows, cand, rel, 30, 1.0, 30, dtype)
    assert r["pos"].tolist() == np.argsort(-rel, kind="stable").tolist()
    assert np.array_equal(r["value"], rel[r["pos"]]) and np.array_equal(r["item"], cand[r["pos"]])
    flat = rref.mmr_query(rows, cand, np.full(30, 0.5, np.float32), 30, 1.0, 5, dtype)
    assert flat["pos"].tolist() == [0, 1, 2, 3, 4]
    # identical rows and rel: every round is a tie among the rest
    same = rref.mmr_query(np.ones((3, 4), np.float32), np.array([2, 2, 1, 0]), np.ones(4, np.float32), 4, 0.5, 4, dtype)
    assert same["pos"].tolist() == [0, 1, 2, 3]


def test_absent_candidates_lengths_and_padding():
    rows = _unit([1, 0, 0, 0], [0, 1, 0, 0])
    cand, rel = np.array([0, 5, 1, -1, 0]), np.array([1.0, 9.0, np.nan, 9.0, np.inf], np.float32)
    r = rref.mmr_query(rows, cand, rel, 5, 0.5, 4, np.float32)
    assert r["pos"].tolist() == [0, -1, -1, -1] and r["item"].tolist() == [0, -1, -1, -1] and r["length"] == 1
    assert r["rel"].tolist() == [1.0, 0, 0, 0] and r["failed"] == rref.FAIL_POS | rref.FAIL_REL
    assert rref.mmr_query(rows, cand, rel, 1, 0.5, 4, np.float32)["failed"] == 0        # what lies behind L is not looked at
    assert rref.mmr_query(rows, cand, rel, 2, 0.5, 4, np.float32)["failed"] == rref.FAIL_POS
    for L in (0, -3):
        r = rref.mmr_query(rows, cand, rel, L, 0.5, 2, np.float32)
        assert r["length"] == 0 and r["pos"].tolist() == [-1, -1] and r["value"].tolist() == [0, 0]
    assert rref.mmr_query(rows, cand, rel, 99, 0.5, 4, np.float32)["length"] == 1       # clamped to the width


def test_ils_by_hand():
    rows = _unit([1, 0, 0, 0], [1, 1, 0, 0], [0, 2, 0, 0], [3, 0, 0, 0])
    cand = np.array([0, 1, 2, 3, 0])
    # sims: (1,0) 1; (2,0) 0, (2,1) 2; (3,0) 3, (3,1) 3, (3,2) 0; (4,.) 1 1 0 3
    ils, valid, failed = rref.ils_query(rows, cand, 5, (1, 2, 3, 4, 5, 9), np.float32)
    assert valid.tolist() == [0, 1, 1, 1, 1, 1] and failed == 0
    assert ils.tolist() == [0, 1.0, 1.0, 1.5, np.float32(14 / 10), np.float32(14 / 10)]
    ils, valid, _ = rref.ils_query(rows, cand, 3, (2, 4), np.float64)
    assert ils.tolist() == [1.0, 1.0] and valid.tolist() == [1, 1]
    # an absent position is not counted: the pairs of the other three
    ils, valid, failed = rref.ils_query(rows, np.array([0, 7, 2, 3]), 4, (2, 4), np.float32)
    assert failed == rref.FAIL_POS and valid.tolist() == [0, 1] and ils.tolist() == [0, 1.0]
    assert rref.ils_query(rows, np.array([0, 7, 2, 3]), 1, (2, 4), np.float32)[2] == 0
    assert rref.ils_query(rows, cand, 0, (2,), np.float32)[1].tolist() == [0]


def test_ils_order_witnesses():
    """sims of 1, 2^53 and -2^53 met in this order give 0 in fp64 and 1 backwards: once inside one row's chain over j, once
    across the prefix over i"""
    ks = (4,)
    cand = np.arange(4)
    a = rref.ils_query(rref.WITNESS_ROW_CHAIN, cand, 4, ks, np.float32)[0]
    b = rref.ils_query(rref.WITNESS_ROW_CHAIN, cand, 4, ks, np.float32, reverse_j=True)[0]
    assert a[0] == 0.0 and b[0] == np.float32(1 / 6)
    cand, ks = np.arange(6), (6,)
    a = rref.ils_query(rref.WITNESS_PREFIX, cand, 6, ks, np.float32)[0]
    b = rref.ils_query(rref.WITNESS_PREFIX, cand, 6, ks, np.float32, reverse_i=True)[0]
    assert a[0] == 0.0 and b[0] == np.float32(1 / 15)
    for rows in (rref.WITNESS_ROW_CHAIN, rref.WITNESS_PREFIX):                       # the witnesses' sims are float32 numbers
        assert np.array_equal(rref.gram_of(rows, np.arange(rows.shape[0])).astype(np.float32),
                              np.stack([rref.sim_rows(rows, r, np.float32) for r in rows]))


# ---- exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 8, 32, 64, 100, 128])
def test_exact_cases_are_exact_in_fp64(D):
    """on exact tables every sim, product and v is a float32 number: the two flavours agree bit for bit, and the sims equal a
    plain fp64 matrix product (any order: nothing rounds)"""
    rng = np.random.default_rng(D)
    rows = rref.exact_table(rng, 50, D)
    cand, rel = rng.integers(0, 50, 33), rref.exact_rel(rng, 33)
    gram = rref.gram_of(rows, cand)
    chain64 = np.stack([rref.sim_rows(rows[cand], rows[c], np.float64) for c in cand])
    chain32 = np.stack([rref.sim_rows(rows[cand], rows[c], np.float32) for c in cand])
    assert np.array_equal(gram, chain64) and np.array_equal(gram, chain32.astype(np.float64)) and rref.is_f32(gram)
    assert np.array_equal(gram, gram.T)
    for lam in (0, 0.25, 0.5, 0.75, 1):
        a = rref.mmr_query(rows, cand, rel, 33, lam, 33, np.float64)
        b = rref.mmr_query(rows, cand, rel, 33, lam, 33, np.float32)
        g = rref.mmr_query(rows, cand, rel, 33, lam, 33, np.float64, gram=gram)
        for key in ("pos", "item", "rel", "length"):
            assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], g[key])
        assert rref.is_f32(a["value"]) and np.array_equal(a["value"], b["value"].astype(np.float64))
        assert np.array_equal(a["value"], g["value"])
        assert all(rref.is_f32(v[np.isfinite(v)]) for v in a["values"])
    a, b = rref.ils_query(rows, cand, 33, (2, 10, 33), np.float64), rref.ils_query(rows, cand, 33, (2, 10, 33), np.float32)
    g = rref.ils_query(rows, cand, 33, (2, 10, 33), np.float64, gram=gram)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[0]), _bits(g[0])) and a[1].tolist() == [1, 1, 1]


def test_the_float32_flavour_rounds_on_random_tables():
    rng = np.random.default_rng(1)
    rows = rng.standard_normal((30, 100)).astype(np.float32)
    a, b = rref.sim_rows(rows, rows[0], np.float64), rref.sim_rows(rows, rows[0], np.float32)
    err = np.abs(a - b.astype(np.float64)).max()
    assert 0 < err < 1e-4
    assert np.array_equal(b, np.array([rref.sim_rows(rows[:1], r, np.float32)[0] for r in rows]))      # symmetric bit for bit


def test_staging_threshold():
    assert rref.staged(512, 64) and not rref.staged(513, 64) and rref.staged(256, 128) and not rref.staged(257, 128)
    assert rref.staged(1024, 32) and not rref.staged(1024, 36) and [rref.lanes(D) for D in (4, 8, 12, 100, 128)] == [1, 2, 4, 32, 32]


# ---- the header, compiled for the host plain and with sanitizers -------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rerank") / ("rerank_rule_host_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "host", "rerank_rule_host.cpp"), "-o", exe],
                   check=True)
    return exe


def _words(a):
    return " ".join("%08x" % v for v in _bits(a).reshape(-1))


def _ints(a):
    return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))


def test_the_header_computes_what_the_restatement_computes(host_program, tmp_path):
    rng = np.random.default_rng(4)
    cases = []
    for D, width in ((4, 1), (4, 7), (8, 33), (32, 20), (100, 40), (128, 65)):
        ni = 30
        for exact in (True, False):
            rows = rref.exact_table(rng, ni, D) if exact else rng.standard_normal((ni, D)).astype(np.float32)
            cand = rng.integers(0, ni, width).astype(np.int32)
            rel = rref.exact_rel(rng, width) if exact else rng.standard_normal(width).astype(np.float32)
            if width > 6:
                cand[3], cand[5] = cand[1], cand[1]                            # a duplicated item
            for L in (-1, 0, 1, width // 2, width, width + 5):
                for lam in (0.0, 0.5, 0.7, 1.0):
                    for n_out in sorted({1, min(2, width), width}):
                        cases.append(("mmr", rows, cand, rel, L, lam, n_out))
                cases.append(("ils", rows, cand, None, L, (1, 2, 10, 64, 2000), None))
        bad_c, bad_r = cand.copy(), rel.copy()
        bad_c[0], bad_r[width - 1] = ni, np.inf
        if width > 6:
            bad_c[4], bad_r[2] = -1, np.nan
        cases.append(("mmr", rows, bad_c, bad_r, -1, 0.5, width))
        cases.append(("mmr", rows, bad_c, rel, -1, 0.5, 1))
        cases.append(("mmr", rows, cand, bad_r, -1, 0.5, width))
        cases.append(("ils", rows, bad_c, None, -1, (2, width), None))
    cases.append(("ils", rref.WITNESS_ROW_CHAIN, np.arange(4), None, -1, (4,), None))
    cases.append(("ils", rref.WITNESS_PREFIX, np.arange(6), None, -1, (6,), None))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for kind, rows, cand, rel, L, lam, n_out in cases:
            ni, D = rows.shape
            if kind == "mmr":
                parts = ["mmr %d %d %d %d %d %s" % (ni, D, cand.size, n_out, L, _words(np.float32(lam))), _words(rows),
                         _ints(cand), _words(rel)]
            else:
                parts = ["ils %d %d %d %d %d %s" % (ni, D, cand.size, L, len(lam), _ints(lam)), _words(rows), _ints(cand)]
            f.write("\n".join(parts) + "\n")
    r = subprocess.run([host_program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "geometry 128 4 1024 8 %d %d %d" % (1 << 30, 1 << 29, rref.STAGE_BYTES)
    at, seen = 1, 0
    for kind, rows, cand, rel, L, lam, n_out in cases:
        LL = cand.size if L < 0 else L
        if kind == "mmr":
            w = rref.mmr_query(rows, cand, rel, LL, lam, n_out, np.float32)
            assert lines[at] == "mmr %d %d %d" % (n_out, w["length"], w["failed"]), (lines[at], at)
            assert [int(x) for x in lines[at + 1].split()] == w["pos"].tolist()
            assert [int(x) for x in lines[at + 2].split()] == w["item"].tolist()
            assert [int(x, 16) for x in lines[at + 3].split()] == _bits(w["rel"]).tolist()
            assert [int(x, 16) for x in lines[at + 4].split()] == _bits(w["value"]).tolist()
            at, seen = at + 5, seen | w["failed"]
        else:
            ils, valid, failed = rref.ils_query(rows, cand, LL, lam, np.float32)
            assert lines[at] == "ils %d %d" % (len(lam), failed), (lines[at], at)
            assert [int(x, 16) for x in lines[at + 1].split()] == _bits(ils).tolist()
            assert [int(x) for x in lines[at + 2].split()] == valid.tolist()
            at, seen = at + 3, seen | failed
    assert at == len(lines) and seen == rref.FAIL_POS | rref.FAIL_REL
    assert lines[-2].split() == ["00000000"] and lines[-5].split() == ["00000000"]          # the two witnesses

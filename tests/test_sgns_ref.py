"""CPU: the NumPy reference of skip-gram with negative sampling (tests/_sgns_ref.py) -- the alias table against its integer
masses, the sampler's histograms by chi-square, the closed-form gradients against central finite differences of the fp64
loss, esr_sgns_sample.h -- the text the kernel compiles -- against the restatement through a stand-alone host program built
plain and with the address and undefined-behaviour sanitizers (tests/host/sgns_sample_host.cpp; no HIP, not loaded into
Python), and learning on the planted corpus, whose fp64 result is the fixture tests/golden/sgns_planted.json."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _sgns_ref as sref
from conftest import GOLDEN, ROOT

def _zipf(ni):
    return np.maximum((1000.0 / np.arange(1, ni + 1) ** 1.1).astype(np.int64), 1)


# ---- the noise table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,counts", [
    ("one", [9]), ("two", [1, 5]), ("three", [4, 4, 4]), ("equal", [7] * 50), ("zipf", _zipf(1000).tolist()),
    ("zeros", [0, 3, 0, 0, 900, 1, 0, 12] * 25), ("lone", [0, 0, 5, 0])])
def test_alias_table_reproduces_the_integer_masses(name, counts):
    from esrecsys_amd import factorization as F
    ni = len(counts)
    masses = sref.noise_masses(counts)
    assert sum(masses) == ni << 32 and all((m >= 1) == (c > 0) for m, c in zip(masses, counts))
    keep, alias = sref.alias_table(masses)
    assert keep.dtype == np.uint32 and alias.dtype == np.int32 and keep.shape == alias.shape == (ni,)
    assert sref.table_masses(keep, alias) == masses                            # exactly
    for n in range(ni):                                                       # mass 0: no keep and nobody's alias
        if masses[n] == 0:
            assert keep[n] == 0 and alias[n] != n and not (alias == n).any()
        assert masses[alias[n]] > 0
    if name in ("three", "equal", "one"):
        assert (alias == np.arange(ni)).all()                                 # every column full
    m2 = F.sgns_noise_masses(np.array(counts))
    k2, a2 = F.sgns_alias_table(m2)
    assert m2.dtype == np.int64 and m2.tolist() == masses and np.array_equal(k2, keep) and np.array_equal(a2, alias)
    want = np.array(counts, np.float64) ** 0.75 * (np.array(counts) > 0)
    assert np.max(np.abs(np.array(masses, np.float64) / (ni * 2.0 ** 32) - want / want.sum())) <= 2.0 ** -30


def test_noise_table_refusals():
    from esrecsys_amd import factorization as F
    for bad in ([], [0, 0], [1, -1], [0.5, 1.0]):
        with pytest.raises(ValueError):
            F.sgns_noise_masses(np.array(bad))
    with pytest.raises(ValueError, match="power"):
        F.sgns_noise_masses(np.array([1, 2]), power=float("nan"))
    with pytest.raises(ValueError, match="sum"):
        F.sgns_alias_table([1, 2, 3])


# ---- the sampler -----------------------------------------------------------------------------------------------------------
def _chi_square_p(observed, expected):
    """the upper tail of the chi-square statistic by the Wilson-Hilferty normal approximation (no scipy)"""
    import math
    observed, expected = np.asarray(observed, np.float64), np.asarray(expected, np.float64)
    stat, df = float(((observed - expected) ** 2 / expected).sum()), observed.size - 1
    z = ((stat / df) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * df))) / math.sqrt(2.0 / (9.0 * df))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


@pytest.mark.parametrize("window,K,seed", [(5, 5, 11), (32, 2, (7 << 32) | 5)])
def test_distance_and_noise_histograms(window, K, seed):
    """2^20 restated slots over one long document: the distances follow window - d + 1, the noise items the masses"""
    ni, n = 200, 1 << 20
    rng = np.random.default_rng(3)
    doc = np.arange(4000) % ni                                                # the distance of a pair can be read off the items
    so, su, si = sref.doc_csr([doc.tolist()])
    counts = rng.integers(0, 50, ni)
    counts[::9] = 0
    masses = sref.noise_masses(counts)
    keep, alias = sref.alias_table(masses)
    c, e, o, valid, neg, dropped = sref.sample_ref(so, su, si, 1, ni, window, K, keep, alias, seed, 0, 1, n)
    c, e, o, valid = c[0], e[0], o[0], valid[0].astype(bool)
    inner = (e >= window) & (e < doc.size - window)                           # both sides inside: nothing dropped there
    assert valid[inner].all() and (~valid).any() and dropped[0] == (~valid).sum()
    d = np.minimum((o - c) % ni, (c - o) % ni)[inner]
    assert d.min() == 1 and d.max() == window
    weights = np.arange(window, 0, -1, dtype=np.float64)
    p_d = _chi_square_p(np.bincount(d, minlength=window + 1)[1:], weights / weights.sum() * d.size)
    right = ((o[inner] - c[inner]) % ni) == d
    p_side = _chi_square_p([right.sum(), (~right).sum()], [d.size / 2, d.size / 2])
    live = np.array(masses) > 0
    hist = np.bincount(neg.reshape(-1), minlength=ni)
    assert not hist[~live].any()                                              # mass 0 is never drawn
    p_n = _chi_square_p(hist[live], np.array(masses, np.float64)[live] / (ni * 2.0 ** 32) * neg.size)
    print("sgns sampler chi-square p: distance %.3g side %.3g noise %.3g" % (p_d, p_side, p_n))
    assert min(p_d, p_side, p_n) > 1e-6


def test_documents_bound_the_context():
    docs = [[0], [1, 2], [3], [4, 5, 6], [7]]
    so, su, si = sref.doc_csr(docs)
    keep, alias = sref.alias_table(sref.noise_masses([1] * 8))
    c, e, o, valid, neg, dropped = sref.sample_ref(so, su, si, 5, 8, 4, 3, keep, alias, 5, 2 ** 32 - 1, 2, 500)
    assert not valid[np.isin(c, (0, 3, 7))].any() and np.array_equal(o[valid == 0], c[valid == 0])     # length 1: dropped
    assert set(zip(c[valid == 1].tolist(), o[valid == 1].tolist())) == {(1, 2), (2, 1), (4, 5), (5, 4), (5, 6), (6, 5), (4, 6),
                                                                       (6, 4)}
    assert np.array_equal(dropped, (valid == 0).sum(1)) and neg.min() >= 0 and neg.max() < 8


# ---- gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_closed_form_gradients_equal_finite_differences(reg):
    rng = np.random.default_rng(0)
    ni, D, B, K = 9, 6, 40, 4
    V, W = 0.5 * rng.standard_normal((ni, D)), 0.5 * rng.standard_normal((ni, D))
    c, o, neg = rng.integers(0, ni, B), rng.integers(0, ni, B), rng.integers(0, ni, (B, K))
    neg[:5, 1] = o[:5]                                                        # n_k == o: skipped
    neg[5:9, 2] = neg[5:9, 0]                                                 # a repeated noise id
    r = sref.fwd_bwd_ref(V, W, c, o, neg, None, reg, np.float64)
    dense_in, dense_out = np.zeros_like(V), np.zeros_like(W)
    np.add.at(dense_in, c, r["centre"])
    np.add.at(dense_out, o, r["positive"])
    for k in range(K):
        np.add.at(dense_out, neg[:, k], r["noise"][k])
    assert not r["noise"][1][:5].any() and r["noise"][0][:5].any()
    h = 1e-6
    for table, dense, which in ((V, dense_in, 0), (W, dense_out, 1)):
        for row, col in ((0, 0), (3, 2), (8, 5), (4, 1)):
            up, down = table.copy(), table.copy()
            up[row, col] += h
            down[row, col] -= h
            args = ((up, W), (down, W)) if which == 0 else ((V, up), (V, down))
            fd = (sref.objective(*args[0], c, o, neg, reg) - sref.objective(*args[1], c, o, neg, reg)) / (2 * h)
            assert abs(fd - dense[row, col]) <= 1e-7 * max(1.0, abs(fd)), (which, row, col, fd, dense[row, col])
    # the loss the kernel reports is the logistic part; valid == 0 and an id outside the table give zeros
    assert abs(r["loss_t"].sum() - sref.objective(V, W, c, o, neg, 0.0)) <= 1e-10
    valid = (np.arange(B) % 3 != 1).astype(np.int32)
    c2 = c.copy()
    c2[3] = ni
    z = sref.fwd_bwd_ref(V, W, c2, o, neg, valid, reg, np.float64)
    off = (valid == 0) | (np.arange(B) == 3)
    assert z["bad"] and not z["loss_t"][off].any() and not z["s"][off].any() and not z["centre"][off].any()
    assert not z["noise"][:, off].any() and np.array_equal(z["centre"][~off], r["centre"][~off])
    f32 = sref.fwd_bwd_ref(V, W, c, o, neg, None, reg, np.float32)
    assert f32["grads"].dtype == np.float32 and sref.arr_err(f32["grads"], r["grads"]) < 1e-5


def test_one_step_moves_only_the_named_rows_and_sgd_is_the_plain_rule():
    rng = np.random.default_rng(6)
    ni, D, B, K = 12, 4, 9, 3
    tables = [rng.standard_normal((ni, D)) for _ in range(2)]
    accums = [np.full_like(t, sref.ACC0) for t in tables]
    c, o, neg = rng.integers(0, 6, B), rng.integers(0, 6, B), rng.integers(0, 6, (B, K))
    for opt in ("adagrad", "sgd"):
        r = sref.step_ref(tables, accums, c, o, neg, None, 0.01, 0.05, opt, np.float64)
        assert np.array_equal(r["in"][6:], tables[0][6:]) and np.array_equal(r["out"][6:], tables[1][6:])
        assert not np.array_equal(r["in"][np.unique(c)], tables[0][np.unique(c)])
    dense = np.zeros_like(tables[1])
    np.add.at(dense, np.concatenate([o, neg.T.reshape(-1)]), r["grads"][B:])
    assert np.max(np.abs(r["out"] - (tables[1] - 0.05 * dense))) <= 1e-15 and np.array_equal(r["out_acc"], accums[1])


# ---- the header, compiled for the host plain and with sanitizers -----------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sgns") / ("sgns_sample_host_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags +
                   [os.path.join(ROOT, "tests", "host", "sgns_sample_host.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_draws_what_the_restatement_draws(host_program, tmp_path):
    (so, su, si), nd, ni, keep, alias = sref.boundary_corpus()
    cases = [((so, su, si), nd, ni, window, K, keep, alias, seed, step0, steps, B) for window, K, seed, step0, steps, B in [
        (1, 1, 5, 0, 2, 300), (5, 5, (0xDEADBEEF << 32) | 7, 2 ** 32 - 2, 3, 257), (32, 16, 2 ** 64 - 1, 123456, 2, 65),
        (32, 3, 9, 1, 1, 64)]]
    k1, a1 = sref.alias_table(sref.noise_masses([4]))
    cases.append((sref.doc_csr([[0]]), 1, 1, 3, 2, k1, a1, 5, 0, 1, 50))          # one event: always dropped
    # ill-formed CSRs: offsets outside the arrays, not ascending; documents outside [0, nd) -- a wrong slot, no wild read
    cases.append(((np.array([5, 2000, -3, 4, 4, 1 << 40, 0, 3]), np.where(np.arange(su.size) % 3 == 0, 99, su - 2), si),
                  nd, ni, 32, 4, keep, alias, 11, 0, 1, 300))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for (o, u, i), n_d, n_i, window, K, kp, al, seed, step0, steps, B in cases:
            f.write("%d %d %d %d %d %d %d %d %d\n" % (n_d, n_i, u.size, window, K, seed, step0, steps, B))
            for a in (o, u, i, kp, al):
                f.write(" ".join(str(int(v)) for v in a) + "\n")
    r = subprocess.run([host_program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "max_window %d max_negatives %d" % (sref.MAX_WINDOW, sref.MAX_NEGATIVES)
    at = 1
    for (o, u, i), n_d, n_i, window, K, kp, al, seed, step0, steps, B in cases:
        assert lines[at] == "case %d %d" % (steps, B)
        got = np.array([l.split() for l in lines[at + 1:at + 1 + steps * B]], dtype=np.int64).reshape(steps, B, 4 + K)
        at += 1 + steps * B
        want = sref.sample_ref(o, u, i, n_d, n_i, window, K, kp, al, seed, step0, steps, B)
        for n in range(4):
            assert np.array_equal(got[:, :, n], want[n]), (n_i, seed, "ceov"[n])
        assert np.array_equal(got[:, :, 4:], want[4]) and (got[:, :, 1] < u.size).all()
    assert at == len(lines)


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_the_reference_learns_the_planted_corpus_and_is_the_fixture():
    P = sref.PLANTED
    indices, offsets = sref.planted_documents()
    assert len(np.unique(indices)) == P["ni"] and offsets[-1] == indices.size
    share, losses = sref.planted_run(np.float64)
    assert len(losses) == P["steps"] and np.isfinite(losses).all() and np.mean(losses[-10:]) < np.mean(losses[:10])
    fixture = json.load(open(os.path.join(GOLDEN, "sgns_planted.json")))
    assert fixture["settings"] == P and fixture["chance"] == 31.0 / 63.0
    print("sgns planted corpus: fp64 own-community share@5 %.3f (fixture %.3f, chance %.3f, bar %.3f)"
          % (share, fixture["own_share_at_5"], fixture["chance"], fixture["bar"]))
    assert abs(share - fixture["own_share_at_5"]) <= 1.0 / (P["ni"] * P["k"]) + 1e-12      # the fixture is this run
    assert fixture["bar"] == fixture["chance"] + 0.5 * (fixture["own_share_at_5"] - fixture["chance"])
    assert share >= fixture["bar"] + 0.5 * (1.0 - fixture["bar"])             # the restatement clears the bar comfortably

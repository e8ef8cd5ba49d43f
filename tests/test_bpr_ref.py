"""CPU: the NumPy reference of BPR (tests/_bpr_ref.py) against torch-CPU autograd in fp64, the stable softplus / sigmoid at
large |d|, the sampler's rule on hand-worked CSRs, esr_bpr_sample.h -- the text the kernel compiles -- against the
restatement through a stand-alone host program built with the address and undefined-behaviour sanitizers
(tests/host/bpr_sample_host.cpp; no HIP, not loaded into Python), and learning on the planted corpus."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _bpr_ref as bref
from conftest import ROOT


# ---- gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_closed_form_gradients_equal_autograd(reg):
    import torch
    rng = np.random.default_rng(0)
    nu, ni, D, B = 7, 9, 12, 40
    U, Y = rng.standard_normal((nu, D)), rng.standard_normal((ni, D))
    u, i, j = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    j[:3] = i[:3]                                                            # i == j: pure regularisation
    valid = (rng.random(B) < 0.8).astype(np.int32)
    loss_t, d, grads = bref.fwd_bwd_ref(U, Y, u, i, j, valid, reg, np.float64)
    tu, ti, tj = (torch.from_numpy(a) for a in (u, i, j))
    x = torch.from_numpy(U)[tu].clone().requires_grad_(True)
    yi = torch.from_numpy(Y)[ti].clone().requires_grad_(True)
    yj = torch.from_numpy(Y)[tj].clone().requires_grad_(True)
    dd = (x * yi).sum(1) - (x * yj).sum(1)
    per = torch.nn.functional.softplus(-dd) + 0.5 * reg * ((x * x).sum(1) + (yi * yi).sum(1) + (yj * yj).sum(1))
    (per * torch.from_numpy(valid).to(torch.float64)).sum().backward()
    want = torch.cat([x.grad, yi.grad, yj.grad]).numpy()
    assert np.max(np.abs(grads - want)) <= 1e-12
    keep = valid != 0
    assert np.max(np.abs(d[keep] - dd.detach().numpy()[keep])) <= 1e-12
    assert np.max(np.abs(loss_t[keep] - torch.nn.functional.softplus(-dd).detach().numpy()[keep])) <= 1e-12
    assert not grads[np.tile(~keep, 3)].any() and not loss_t[~keep].any() and not d[~keep].any()
    if reg == 0.0:
        assert not grads[:3].any()                                           # i == j without reg: no gradient at all


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_softplus_and_sigmoid_are_finite_and_correct_at_large_d(dtype):
    d = np.array([-100.0, -20.0, 0.0, 20.0, 100.0], dtype)
    with np.errstate(over="raise", invalid="raise", divide="raise"):         # (e^-100 underflows in float32: harmless)
        sp, sg = bref.softplus_neg(d), bref.sigmoid_neg(d)
    assert sp.dtype == dtype and sg.dtype == dtype and np.isfinite(sp).all() and np.isfinite(sg).all()
    import math
    want_sp = [100.0, 20.0 + math.log1p(math.exp(-20.0)), math.log(2.0), math.log1p(math.exp(-20.0)), math.exp(-100.0)]
    want_sg = [1.0, 1.0 / (1.0 + math.exp(-20.0)), 0.5, math.exp(-20.0) / (1.0 + math.exp(-20.0)), math.exp(-100.0)]
    tol = 4 * np.finfo(dtype).eps
    for got, want in ((sp, want_sp), (sg, want_sg)):
        for a, b in zip(got.astype(np.float64), want):
            assert abs(a - b) <= tol * b + (1e-45 if dtype == np.float32 else 0.0), (a, b)
    assert sp[4] > 0 or dtype == np.float32                                  # e^-100 is below float32's subnormals
    assert sg[0] == 1 and sg[2] == 0.5 and sp[0] == 100


# ---- the sampler on hand-worked CSRs ---------------------------------------------------------------------------------------
def _draw(csr, nu, ni, seed=5, step0=0, K=2, B=300):
    return bref.sample_ref(*csr, nu, ni, seed, step0, K, B)


def test_all_items_but_one_seen():
    ni = 6
    csr = bref.csr_of({0: [0, 1, 2, 4, 5], 1: [3]}, 2)                     # user 0 has not seen item 3 alone
    u, i, j, valid, dropped = _draw(csr, 2, ni)
    assert set(np.unique(u)) == {0, 1} and ((valid == 0) | (valid == 1)).all()
    ok0 = (u == 0) & (valid == 1)
    assert ok0.any() and (j[ok0] == 3).all()
    assert (i[u == 1] == 3).all() and (j[(u == 1) & (valid == 1)] != 3).all()
    assert set(i[u == 0]) <= {0, 1, 2, 4, 5}
    # a dropped triple carries its last candidate, a seen item
    bad = valid == 0
    assert (j[bad & (u == 0)] != 3).all()
    assert np.array_equal(dropped, bad.sum(1)) and dropped.dtype == np.int32
    # (5 / 6)^15 = 6.5 % of user 0's triples are dropped: some are, in 600 draws
    assert bad.any()


def test_a_user_who_has_seen_everything_is_always_dropped():
    csr = bref.csr_of({0: [0, 1, 2]}, 1)
    u, i, j, valid, dropped = _draw(csr, 1, 3, K=2, B=50)
    assert not valid.any() and list(dropped) == [50, 50] and not u.any() and set(np.unique(j)) <= {0, 1, 2}


def test_one_item_and_one_pair():
    u, i, j, valid, dropped = _draw(bref.csr_of({0: [0], 1: []}, 2), 2, 1, K=1, B=20)          # ni = 1: the item is seen
    assert not valid.any() and not j.any() and not i.any() and not u.any() and list(dropped) == [20]
    u, i, j, valid, dropped = _draw(bref.csr_of({2: [4]}, 3), 3, 9, K=1, B=64)                 # nnz = 1
    assert (u == 2).all() and (i == 4).all() and valid.all() and (j != 4).all() and not dropped.any()
    assert len(np.unique(j)) > 4


def test_the_rule_word_by_word():
    """slot t of step s: block b = philox((t, s, b, 0), (seed lo, seed hi)); word 0 of block 0 the pair, then candidates"""
    from _spotify_sampler_ref import philox4x32_10
    rng = np.random.default_rng(2)
    nu, ni = 5, 11
    off, upos, ipos = bref.random_csr(rng, nu, ni, (1, 4, 9, 10, 2))
    seed, s = (0xDEADBEEF << 32) | 0x1234, 7
    u, i, j, valid, _ = bref.sample_ref(off, upos, ipos, nu, ni, seed, s - 1, 2, 40)
    for t in range(40):
        words = np.concatenate([philox4x32_10([t, s, b, 0], [0x1234, 0xDEADBEEF]) for b in range(4)]).astype(np.uint64)
        p = int(words[0]) * upos.size >> 32
        assert (u[1, t], i[1, t]) == (upos[p], ipos[p])
        row = set(ipos[off[upos[p]]:off[upos[p] + 1]].tolist())
        cands = [int(w) * ni >> 32 for w in words[1:]]
        assert len(cands) == bref.MAX_TRIES
        fresh = [c for c in cands if c not in row]
        assert valid[1, t] == bool(fresh) and j[1, t] == (fresh[0] if fresh else cands[-1])


def test_a_seed_with_a_high_word_and_the_step_and_slot_enter():
    rng = np.random.default_rng(3)
    csr = bref.random_csr(rng, 20, 50, (3, 7))
    lo = 0x9E3779B9
    a = _draw(csr, 20, 50, seed=lo, K=1, B=64)
    b = _draw(csr, 20, 50, seed=lo | (1 << 32), K=1, B=64)
    c = _draw(csr, 20, 50, seed=lo + (1 << 64), K=1, B=64)                  # seeds are taken mod 2^64
    assert not np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a, c))
    # row k of a K = 3 call is the K = 1 call at step0 + k (the step counter wraps at 2^32); a longer batch extends a shorter
    full = _draw(csr, 20, 50, step0=2 ** 32 - 2, K=3, B=70)
    for k in range(3):
        one = _draw(csr, 20, 50, step0=(2 ** 32 - 2 + k) % 2 ** 32, K=1, B=64)
        assert all(np.array_equal(x[k, :64], y[0]) for x, y in zip(full[:4], one[:4]))
    assert not np.array_equal(full[2][0], full[2][1])


def test_bias_bounds_are_stated_in_the_header():
    text = open(os.path.join(ROOT, "esrecsys_amd", "csrc", "esr_bpr_sample.h")).read()
    assert "nnz / 2^32" in text and "ni / 2^32" in text and "kBprMaxTries = 15" in text


# ---- the header, compiled for the host with sanitizers -----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("bpr") / "bpr_sample_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "bpr_sample_host.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_draws_what_the_restatement_draws(host_program, tmp_path):
    rng = np.random.default_rng(4)
    cases = [  # (csr, nu, ni, seed, step0, K, B)
        (bref.csr_of({0: [0, 1, 2, 4, 5], 1: [3]}, 2), 2, 6, 5, 0, 2, 300),
        (bref.csr_of({0: [0, 1, 2]}, 1), 1, 3, 5, 0, 2, 50),
        (bref.csr_of({0: [0], 1: []}, 2), 2, 1, 5, 0, 1, 20),
        (bref.csr_of({2: [4]}, 3), 3, 9, 5, 0, 1, 64),
        (bref.random_csr(rng, 20, 50, (3, 7)), 20, 50, (0xDEADBEEF << 32) | 7, 2 ** 32 - 2, 3, 70),
        (bref.random_csr(rng, 9, 1001, (1, 2, 63, 64, 65, 1000)), 9, 1001, 2 ** 64 - 1, 123456, 2, 257),
        (bref.random_csr(rng, 300, 40, (0, 1, 39, 40)), 300, 40, 1 << 32, 1, 1, 500),
    ]
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for (off, upos, ipos), nu, ni, seed, step0, K, B in cases:
            f.write("%d %d %d %d %d %d %d\n" % (nu, ni, upos.size, seed, step0, K, B))
            for a in (off, upos, ipos):
                f.write(" ".join(str(int(v)) for v in a) + "\n")
    r = subprocess.run([host_program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "max_tries %d" % bref.MAX_TRIES
    at = 1
    for (csr, nu, ni, seed, step0, K, B) in cases:
        assert lines[at] == "case %d %d" % (K, B)
        got = np.array([l.split() for l in lines[at + 1:at + 1 + K * B]], dtype=np.int64).reshape(K, B, 4)
        at += 1 + K * B
        u, i, j, valid, _ = bref.sample_ref(*csr, nu, ni, seed, step0, K, B)
        for n, want in enumerate((u, i, j, valid)):
            assert np.array_equal(got[:, :, n], want), (nu, ni, seed, "uijv"[n])
    assert at == len(lines)


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_the_reference_learns_the_planted_communities():
    user, item = bref.planted_pairs()
    assert user.size == 64 * 8 and len(set(zip(user.tolist(), item.tolist()))) == user.size
    assert ((item >= 32) == (user >= 32)).all()
    losses = bref.planted_losses(np.float64)
    assert len(losses) == 60 and np.isfinite(losses).all()
    assert np.mean(losses[-10:]) < np.mean(losses[:10]), (losses[:10], losses[-10:])


def test_one_step_moves_only_the_named_rows_and_sgd_is_the_plain_rule():
    rng = np.random.default_rng(6)
    nu, ni, D, B = 10, 12, 4, 9
    U, Y = rng.standard_normal((nu, D)), rng.standard_normal((ni, D))
    Ua, Ya = np.full_like(U, bref.ACC0), np.full_like(Y, bref.ACC0)
    u, i, j = rng.integers(0, 5, B), rng.integers(0, 6, B), rng.integers(0, 6, B)
    valid = np.ones(B, np.int32)
    for opt in ("adagrad", "sgd"):
        r = bref.step_ref(U, Y, Ua, Ya, u, i, j, valid, 0.01, 0.05, opt, np.float64)
        assert np.array_equal(r["user"][5:], U[5:]) and np.array_equal(r["item"][6:], Y[6:])
        assert not np.array_equal(r["user"][np.unique(u)], U[np.unique(u)])
    dense = np.zeros_like(Y)
    np.add.at(dense, np.concatenate([i, j]), r["grads"][B:])
    assert np.max(np.abs(r["item"] - (Y - 0.05 * dense))) <= 1e-15
    assert np.array_equal(r["item_acc"], Ya)

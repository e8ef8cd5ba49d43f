"""CPU: the NumPy reference of FPMC (tests/_fpmc_ref.py) against torch-CPU autograd in fp64 on the loss and all 5 + c
gradient rows, the sampler's rule on hand-worked sequences, esr_fpmc_sample.h -- the text the kernel compiles -- against the
restatement through a stand-alone host program built with the address and undefined-behaviour sanitizers
(tests/host/fpmc_sample_host.cpp; no HIP, not loaded into Python), and learning on the planted chain, whose fp64 hit rate
is the fixture tests/golden/fpmc_planted.json that the GPU test reads."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _fpmc_ref as fref
from conftest import GOLDEN, ROOT


# ---- gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.01])
def test_closed_form_gradients_equal_autograd(reg):
    import torch
    rng = np.random.default_rng(0)
    nu, ni, D, B = 7, 9, 12, 60
    U, A, Bn, P = (0.5 * rng.standard_normal((n, D)) for n in (nu, ni, ni, ni))      # (|d| stays below softplus's threshold)
    seq = rng.integers(0, ni, 40)
    seq[10:13] = 4                                                           # a context with a repeated item
    e = rng.integers(0, seq.size, B)
    c = np.minimum(e, rng.integers(0, 9, B))
    e[0], c[0] = 13, 3                                                       # the context 4, 4, 4
    u, i, j = rng.integers(0, nu, B), seq[e], rng.integers(0, ni, B)
    j[:3] = i[:3]                                                            # i == j: pure regularisation
    e[5], c[5] = 20, 8
    i[5] = seq[15]                                                           # i inside its own context
    c[7] = 0
    valid = (rng.random(B) < 0.8).astype(np.int32)
    valid[[0, 1, 5, 7]] = 1
    loss_t, d, grads, ctx_ids = fref.fwd_bwd_ref(U, A, Bn, P, seq, u, e, c, i, j, valid, reg, np.float64)
    M = int(c.sum())
    assert grads.shape == (5 * B + M, D) and ctx_ids.shape == (M,)
    off = np.concatenate([[0], np.cumsum(c)])
    leaf = lambda a: torch.from_numpy(a).clone().requires_grad_(True)          # noqa: E731
    x, ai, aj, bi, bj = leaf(U[u]), leaf(A[i]), leaf(A[j]), leaf(Bn[i]), leaf(Bn[j])
    want_ids = np.concatenate([seq[e[t] - c[t]:e[t]] for t in range(B)])
    assert np.array_equal(ctx_ids, want_ids)
    pc = leaf(P[want_ids])                                                   # one leaf row per context occurrence
    m = torch.stack([pc[off[t]:off[t + 1]].sum(0) / max(int(c[t]), 1) for t in range(B)])
    dd = (x * ai).sum(1) + (m * bi).sum(1) - (x * aj).sum(1) - (m * bj).sum(1)
    sq = lambda r: (r * r).sum(1)                                              # noqa: E731
    l2 = sq(x) + sq(ai) + sq(aj) + sq(bi) + sq(bj) + torch.stack([sq(pc[off[t]:off[t + 1]]).sum() for t in range(B)])
    per = torch.nn.functional.softplus(-dd) + 0.5 * reg * l2
    (per * torch.from_numpy(valid).to(torch.float64)).sum().backward()
    want = torch.cat([x.grad, ai.grad, aj.grad, bi.grad, bj.grad, pc.grad]).numpy()
    assert np.max(np.abs(grads - want)) <= 1e-12
    keep = valid != 0
    assert np.max(np.abs(d[keep] - dd.detach().numpy()[keep])) <= 1e-12
    assert np.max(np.abs(loss_t[keep] - torch.nn.functional.softplus(-dd).detach().numpy()[keep])) <= 1e-12
    assert not grads[:5 * B][np.tile(~keep, 5)].any() and not loss_t[~keep].any() and not d[~keep].any()
    assert not grads[5 * B:][np.repeat(~keep, c)].any() and (~keep).any()
    if reg == 0.0:
        assert not grads[:3].any() and not grads[5 * B + off[0]:5 * B + off[3]].any()      # i == j without reg: nothing
        assert not grads[3 * B + 7].any() and grads[B + 7].any()             # c = 0: the user-item term alone
    else:
        assert np.array_equal(grads[3 * B + 7], reg * Bn[i[7]])              # c = 0: the Bn rows are the L2 term alone


def test_refused_slots_give_zeros_and_keep_the_layout():
    rng = np.random.default_rng(1)
    nu, ni, D = 4, 5, 8
    U, A, Bn, P = (rng.standard_normal((n, D)) for n in (nu, ni, ni, ni))
    seq = np.array([0, 1, 9, 3, 4, 2, -1, 1])                                # events 2 and 6 name no item
    u = np.array([0, nu, 1, 2, 3, 0, 1]); e = np.array([1, 2, 4, 5, 7, 8, 1]); c = np.array([1, 2, 2, 1, 3, 1, 2])
    i = np.array([1, 1, ni, 2, 1, 1, 1]); j = np.array([2, 2, 2, -1, 2, 2, 2])
    loss_t, d, grads, ctx_ids = fref.fwd_bwd_ref(U, A, Bn, P, seq, u, e, c, i, j, None, 0.01, np.float64)
    B = u.size
    assert loss_t[0] > 0 and not loss_t[1:].any() and not d[1:].any()        # u, i, j, a context id, e and c > e in turn
    assert not grads[1:B].any() and not grads[5 * B + 1:].any() and grads[5 * B].any()
    assert ctx_ids.tolist() == [0, 0, 1, 0, 3, 4, 4, 2, 0, 0, 0, 0]


# ---- the sampler on hand-worked sequences ------------------------------------------------------------------------------------
def _draw(seqs, nu, ni, window, seed=5, step0=0, K=2, B=400):
    (so, su, si), (ro, ri) = fref.seq_csr(seqs, nu)
    return fref.sample_ref(so, su, si, ro, ri, nu, ni, window, seed, step0, K, B), (so, su, si)


@pytest.mark.parametrize("window", [1, 3, 8])
def test_context_lengths_and_user_boundaries(window):
    """lengths 1, 2, window and window + 1; a user of length 1 directly before another user; an empty user"""
    ni = 40
    seqs = {0: [7], 1: [3, 3], 2: list(range(10, 10 + window)), 3: [], 4: [9], 5: list(range(20, 21 + window)), 6: [1], 7: [2, 5]}
    (u, e, c, i, j, valid, dropped), (so, su, si) = _draw(seqs, 8, ni, window)
    assert set(np.unique(u)) == {0, 1, 2, 4, 5, 6, 7}                       # the empty user is never drawn
    pos = e - so[u]
    assert np.array_equal(c, np.minimum(pos, window)) and (e - c >= so[u]).all()        # the context stays in u's events
    assert np.array_equal(i, si[e]) and np.array_equal(u, su[e])
    assert not c[(u == 0) | (u == 4) | (u == 6)].any()                       # length 1: no context, whoever comes before
    assert set(c[u == 1]) == {0, 1} and set(c[u == 7]) == {0, 1}
    assert set(c[u == 2]) == set(range(window)) and set(c[u == 5]) == set(range(window + 1))
    assert (c[u == 5].max() == window) and (pos[u == 5].max() == window)
    seen = {k: set(v) for k, v in seqs.items()}
    assert all(jj not in seen[uu] for uu, jj, ok in zip(u.ravel(), j.ravel(), valid.ravel()) if ok)
    assert np.array_equal(dropped, (valid == 0).sum(1)) and dropped.dtype == np.int32


def test_negatives_are_bprs_and_repeats_are_kept():
    import _bpr_ref as bref
    seqs = {0: [2, 2, 2, 5, 2], 1: [0, 1, 2, 3, 4, 5, 6], 2: [6]}
    (u, e, c, i, j, valid, dropped), (so, su, si) = _draw(seqs, 3, 8, 2, seed=(9 << 32) | 1, step0=2 ** 32 - 1, K=2, B=300)
    assert si.tolist()[:5] == [2, 2, 2, 5, 2] and so.tolist() == [0, 5, 12, 13]
    # the same Philox words: BPR's sampler over a CSR with as many pairs as there are events draws the same negatives
    # wherever it lands on the same user -- here: one user, so every slot
    one = {0: [0, 1, 2, 4, 5]}
    (_, _, _, _, j1, v1, _), _ = _draw(one, 1, 6, 1, seed=5, K=1, B=200)
    _, _, jb, vb, _ = bref.sample_ref(*bref.csr_of(one, 1), 1, 6, 5, 0, 1, 200)
    assert np.array_equal(j1, jb) and np.array_equal(v1, vb) and (~vb.astype(bool)).any()
    assert (valid[u == 1] == (j[u == 1] == 7)).all()                         # user 1 has seen all but item 7


def test_rows_and_prefixes_do_not_depend_on_the_call():
    seqs = {u: list(np.random.default_rng(u).integers(0, 30, n)) for u, n in enumerate((1, 2, 3, 4, 8, 9, 50))}
    full, _ = _draw(seqs, 7, 30, 3, step0=2 ** 32 - 2, K=3, B=70)
    for k in range(3):
        one, _ = _draw(seqs, 7, 30, 3, step0=(2 ** 32 - 2 + k) % 2 ** 32, K=1, B=64)
        assert all(np.array_equal(x[k, :64], y[0]) for x, y in zip(full[:6], one[:6]))
    a, _ = _draw(seqs, 7, 30, 3, seed=7, K=1, B=64)
    b, _ = _draw(seqs, 7, 30, 3, seed=7 | (1 << 32), K=1, B=64)
    assert not np.array_equal(a[1], b[1])                                    # the high word of the seed enters
    w1, _ = _draw(seqs, 7, 30, 1, K=1, B=64)
    w8, _ = _draw(seqs, 7, 30, 8, K=1, B=64)
    assert all(np.array_equal(x, y) for n, (x, y) in enumerate(zip(w1, w8)) if n != 2)      # the window enters c alone
    assert np.array_equal(w1[2], np.minimum(w8[2], 1))


# ---- the header, compiled for the host with sanitizers -----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fpmc") / "fpmc_sample_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "fpmc_sample_host.cpp"), "-o", exe], check=True)
    return exe


def test_the_header_draws_what_the_restatement_draws(host_program, tmp_path):
    rng = np.random.default_rng(4)
    lengths = (1, 2, 3, 4, 8, 9, 1000)
    big = {u: rng.integers(0, 1001, n).tolist() for u, n in enumerate(lengths)}
    cases = []   # ((seq csr), (seen csr), nu, ni, window, seed, step0, K, B)
    for seqs, nu, ni, window, seed, step0, K, B in [
            ({0: [7], 1: [3, 3], 2: [10, 11, 12], 3: [], 4: [9], 5: [20, 21, 22, 23], 6: [1]}, 7, 40, 3, 5, 0, 2, 300),
            ({0: [0, 1, 2]}, 1, 3, 1, 5, 0, 2, 50),                          # everything seen: always dropped
            ({2: [4]}, 3, 9, 8, 5, 0, 1, 64),                                # one event
            (big, 7, 1001, 1, (0xDEADBEEF << 32) | 7, 2 ** 32 - 2, 3, 70),
            (big, 7, 1001, 8, 2 ** 64 - 1, 123456, 2, 257)]:
        cases.append(fref.seq_csr(seqs, nu) + (nu, ni, window, seed, step0, K, B))
    # ill-formed CSRs: offsets outside the arrays, not ascending; user positions outside [0, nu) -- a wrong slot, no wild read
    (so, su, si), (ro, ri) = fref.seq_csr(big, 7)
    cases.append(((np.array([5, 2000, -3, 4, 4, 1 << 40, 0, 3]), np.where(np.arange(su.size) % 3 == 0, 99, su - 2), si),
                  (np.array([-7, 3, 2, 1 << 40, 0, 5, 5, 5000]), ri), 7, 1001, 8, 11, 0, 1, 300))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for (so, su, si), (ro, ri), nu, ni, window, seed, step0, K, B in cases:
            f.write("%d %d %d %d %d %d %d %d %d\n" % (nu, ni, su.size, ri.size, window, seed, step0, K, B))
            for a in (so, su, si, ro, ri):
                f.write(" ".join(str(int(v)) for v in a) + "\n")
    r = subprocess.run([host_program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "max_window %d max_tries %d" % (fref.MAX_WINDOW, fref.MAX_TRIES)
    at = 1
    for (so, su, si), (ro, ri), nu, ni, window, seed, step0, K, B in cases:
        assert lines[at] == "case %d %d" % (K, B)
        got = np.array([l.split() for l in lines[at + 1:at + 1 + K * B]], dtype=np.int64).reshape(K, B, 6)
        at += 1 + K * B
        want = fref.sample_ref(so, su, si, ro, ri, nu, ni, window, seed, step0, K, B)
        for n in range(6):
            assert np.array_equal(got[:, :, n], want[n]), (nu, ni, seed, "uecijv"[n])
        assert (got[:, :, 2] <= got[:, :, 1]).all() and (got[:, :, 1] < su.size).all()
    assert at == len(lines)


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_split_last_restatement():
    ids = np.array([5, 6, 7, 1, 2, 9, 9, 9, 9, 3], np.int64)
    off = np.array([0, 3, 5, 5, 9, 10])
    ctx, co, truth, to, kept = fref.split_last_ref(ids, off)
    assert ctx.tolist() == [5, 6, 9, 9, 9] and co.tolist() == [0, 2, 5] and truth.tolist() == [7, 9] and kept.tolist() == [0, 3]
    ctx, co, truth, to, kept = fref.split_last_ref(ids, off, n_last=2, min_length=4)
    assert ctx.tolist() == [9, 9] and truth.tolist() == [9, 9] and to.tolist() == [0, 2] and kept.tolist() == [3]


def test_the_reference_learns_the_planted_chain_and_is_the_fixture():
    P = fref.PLANTED
    indices, offsets = fref.planted_sequences()
    seqs = indices.reshape(P["nu"], P["length"])
    follows = ((seqs[:, 1:] - seqs[:, :-1]) % P["ni"] == 1).mean()
    assert 0.85 < follows < 0.95 and len(np.unique(indices)) == P["ni"]
    hit, losses = fref.planted_hit_rate(np.float64)
    assert len(losses) == P["steps"] and np.isfinite(losses).all() and np.mean(losses[-10:]) < np.mean(losses[:10])
    fixture = json.load(open(os.path.join(GOLDEN, "fpmc_planted.json")))
    assert {k: fixture["settings"][k] for k in P} == P and fixture["chance"] == P["k"] / P["ni"]
    print("fpmc planted chain: fp64 hit rate@10 %.3f (fixture %.3f, chance %.3f)" % (hit, fixture["hit_rate_at_10"],
                                                                                  fixture["chance"]))
    assert abs(hit - fixture["hit_rate_at_10"]) <= 1.0 / P["nu"] + 1e-12      # the fixture is this run (one user of slack)
    assert fixture["hit_rate_at_10"] > 4 * fixture["chance"]                 # and far from chance


def test_one_step_moves_only_the_named_rows_and_sgd_is_the_plain_rule():
    rng = np.random.default_rng(6)
    nu, ni, D = 10, 12, 4
    seq = rng.integers(0, 6, 30)
    tables = {k: rng.standard_normal((nu if k == "user" else ni, D)) for k in fref.TABLES}
    accums = {k: np.full_like(v, fref.ACC0) for k, v in tables.items()}
    e = rng.integers(3, 30, 9)
    c, u, i, j = np.minimum(e, 2), rng.integers(0, 5, 9), seq[e], rng.integers(0, 6, 9)
    for opt in ("adagrad", "sgd"):
        r = fref.step_ref(tables, accums, seq, u, e, c, i, j, None, 0.01, 0.05, opt, np.float64)
        assert np.array_equal(r["user"][5:], tables["user"][5:])
        assert all(np.array_equal(r[k][6:], tables[k][6:]) for k in ("item", "next", "prev"))
        assert not np.array_equal(r["prev"][np.unique(r["ctx_ids"])], tables["prev"][np.unique(r["ctx_ids"])])
    dense = np.zeros_like(tables["prev"])
    np.add.at(dense, r["ctx_ids"], r["grads"][45:])
    assert np.max(np.abs(r["prev"] - (tables["prev"] - 0.05 * dense))) <= 1e-15
    assert np.array_equal(r["prev_acc"], accums["prev"])

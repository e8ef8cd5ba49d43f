"""CPU: the NumPy restatement of the bag rules and of the hybrid BPR step (tests/_hybrid_ref.py) -- the step's gradient
against torch-CPU autograd of the stated objective in fp64, hand-worked bags, esr_bag_rule.h (the text the kernels compile)
against the restatement through a stand-alone host program built plain and with the address and undefined-behaviour
sanitizers (tests/host/bag_rule_host.cpp; no HIP, not loaded into Python), and learning on the planted corpus."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _hybrid_ref as href
from conftest import ROOT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the objective -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.01])
@pytest.mark.parametrize("weighted", [False, True])
def test_step_gradient_equals_autograd_of_the_stated_objective(reg, weighted):
    import torch
    rng = np.random.default_rng(0)
    nu, ni, nfu, nfi, D, B = 6, 8, 9, 11, 8, 40
    ue, ie = rng.standard_normal((nfu, D)), rng.standard_normal((nfi, D))

    def bags(n, nf):
        lens = rng.integers(0, 4, n)
        lens[0] = 0                                                          # an empty bag
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        feat = np.concatenate([rng.choice(nf, l, replace=False) for l in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
        w = (rng.standard_normal(feat.size).astype(np.float32)) if weighted else None
        return off, feat, w

    ubag, ibag = bags(nu, nfu), bags(ni, nfi)
    u, i, j = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    u[0], i[1] = 0, 0
    valid = (rng.random(B) < 0.8).astype(np.int32)
    r = href.step_ref(ue, ie, np.ones_like(ue), np.ones_like(ie), ubag, ibag, u, i, j, valid, reg, 0.05, "sgd", np.float64)
    got_u = href.dense_gradient(nfu, r["user_feat"], r["user_grads"])
    got_i = href.dense_gradient(nfi, r["item_feat"], r["item_grads"])

    tu, ti = torch.from_numpy(ue).requires_grad_(True), torch.from_numpy(ie).requires_grad_(True)

    def compose(table, bag, rows):
        off, feat, w = bag
        out, l2 = [], []
        for b in rows:
            k = slice(int(off[b]), int(off[b + 1]))
            e = table[torch.from_numpy(feat[k].astype(np.int64))]
            ww = torch.ones(e.shape[0], dtype=torch.float64) if w is None else torch.from_numpy(w[k].astype(np.float64))
            out.append((ww[:, None] * e).sum(0))
            l2.append((e * e).sum())
        return torch.stack(out), torch.stack(l2)

    x, lx = compose(tu, ubag, u)
    yi, li = compose(ti, ibag, i)
    yj, lj = compose(ti, ibag, j)
    d = (x * yi).sum(1) - (x * yj).sum(1)
    reg32 = float(np.float32(reg))
    per = torch.nn.functional.softplus(-d) + 0.5 * reg32 * (lx + li + lj)
    (per * torch.from_numpy(valid).to(torch.float64)).sum().backward()
    assert np.max(np.abs(got_u - tu.grad.numpy())) <= 1e-12
    assert np.max(np.abs(got_i - ti.grad.numpy())) <= 1e-12
    keep = valid != 0
    assert np.max(np.abs(r["loss_t"][keep] - torch.nn.functional.softplus(-d).detach().numpy()[keep])) <= 1e-12
    # the SGD step is the plain rule on the segment sums
    assert np.max(np.abs(r["item"] - (ie - 0.05 * got_i))) <= 1e-15


def test_identity_only_bags_give_bpr_itself():
    import _bpr_ref as bref
    rng = np.random.default_rng(1)
    nu, ni, D, B = 7, 9, 12, 30
    U, Y = rng.standard_normal((nu, D)), rng.standard_normal((ni, D))
    u, i, j = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    valid = (rng.random(B) < 0.8).astype(np.int32)
    a = href.step_ref(U, Y, np.full_like(U, 0.1), np.full_like(Y, 0.1), href.identity_bags(nu), href.identity_bags(ni), u, i, j,
                      valid, 2.0 ** -7, 0.05, "adagrad", np.float64)   # (a reg that float32 holds: the kernels take a float)
    b = bref.step_ref(U, Y, np.full_like(U, 0.1), np.full_like(Y, 0.1), u, i, j, valid, 2.0 ** -7, 0.05, "adagrad", np.float64)
    for key in ("user", "item", "user_acc", "item_acc"):
        assert np.max(np.abs(a[key] - b[key])) <= 1e-12, key
    assert abs(a["loss"] - b["loss"]) <= 1e-12


# ---- hand-worked bags --------------------------------------------------------------------------------------------------------
def _one_bag(values, weights=None, D=4):
    table = np.repeat(np.array(values, np.float32)[:, None], D, 1)
    off, feat = np.array([0, len(values)], np.int64), np.arange(len(values), dtype=np.int32)
    return href.bag_sum_ref(table, off, feat, weights, None, np.float32)[0][0]


def test_hand_worked_bags():
    big = 2.0 ** 25
    # the issue's bag: 2^25 + 1 rounds back to 2^25 (its ulp is 4), so the stated order gives 0; an order that cancels the
    # two large terms first keeps the 1
    assert _one_bag([big, 1.0, -big]).tolist() == [0.0] * 4
    assert _one_bag([big, -big, 1.0]).tolist() == [1.0] * 4
    # the witness of the grid: 0 in the stated order, 1 when the chain runs backwards
    assert _one_bag(href.WITNESS).tolist() == [0.0] * 4 and _one_bag(href.WITNESS[::-1]).tolist() == [1.0] * 4
    # weights enter the product: (2, 0.5) . (3, 4) = 8
    assert _one_bag([3.0, 4.0], np.array([2.0, 0.5], np.float32)).tolist() == [8.0] * 4
    # an empty bag is a zero row of +0.0; an identity-only bag returns the row itself, bit for bit
    rng = np.random.default_rng(2)
    table = rng.standard_normal((5, 8)).astype(np.float32)
    table[3, 0] = -0.0
    off, feat = np.array([0, 0, 1, 2], np.int64), np.array([3, 1], np.int32)
    for dtype in (np.float32, np.float64):
        out, failed = href.bag_sum_ref(table, off, feat, None, None, dtype)
        assert not failed and not out[0].any() and not np.signbit(out[0]).any()
        assert np.array_equal(out[1].astype(np.float32)[1:], table[3][1:]) and np.array_equal(out[2].astype(np.float32), table[1])
    # -0.0 + +0.0 = +0.0: the chain starts from +0.0f, so a row's -0.0 comes out as +0.0
    assert not np.signbit(href.bag_sum_ref(table, off, feat, None, None, np.float32)[0][1, 0])
    # rows select, repeat and refuse
    out, failed = href.bag_sum_ref(table, off, feat, None, [2, 0, 2, 3, -1], np.float32)
    assert failed and np.array_equal(out[0], table[1]) and np.array_equal(out[2], table[1]) and not out[[1, 3, 4]].any()
    out, failed = href.bag_sum_ref(table, off, np.array([3, 5], np.int32), None, None, np.float32)
    assert failed and not out[2].any() and out[1, 1:].any()


def test_expand_by_hand():
    table = np.arange(12, dtype=np.float32).reshape(3, 4)
    off, feat, w = np.array([0, 2, 2, 3], np.int64), np.array([2, 0, 1], np.int32), np.array([2.0, -1.0, 0.5], np.float32)
    g = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.float32)
    f, rows, oo, failed = href.bag_expand_ref(table, off, feat, w, [0, 1, 2], g, [1, 1, 0], 0.5, np.float32)
    assert not failed and oo.tolist() == [0, 2, 2, 3] and f.tolist() == [2, 0, 1]
    assert rows[0].tolist() == (2.0 * g[0] + 0.5 * table[2]).tolist()
    assert rows[1].tolist() == (-1.0 * g[0] + 0.5 * table[0]).tolist()
    assert not rows[2].any()                                                 # valid = 0: zeros, the position is still named
    f, rows, oo, failed = href.bag_expand_ref(table, off, feat, None, [2, 7, 2], g, None, 0.0, np.float64)
    assert failed and oo.tolist() == [0, 1, 1, 2] and rows[0].tolist() == g[0].tolist() and rows[1].tolist() == g[2].tolist()


def test_exact_cases_are_exact_in_fp64():
    """on the exact tables the two flavours agree wherever float32 holds the sum: the fp64 chain never rounds"""
    rng = np.random.default_rng(3)
    table = href.exact_table(rng, 40, 8)
    off, feat, w = href.grid_bags(rng, 16, 40)
    lens = np.diff(off)
    assert set(lens.tolist()) == set(href.LENGTHS) and lens.max() > 1024 and lens.min() == 0
    a, _ = href.bag_sum_ref(table, off, feat, w, None, np.float64)
    # every fp64 value is a multiple of 2^-9 below 2^40: 49 bits
    assert np.array_equal(a * 512, np.round(a * 512)) and np.abs(a).max() < 2.0 ** 40
    b, _ = href.bag_sum_ref(table, off, feat, w, None, np.float32)
    short = lens <= 2
    assert np.array_equal(a[short], b[short].astype(np.float64))
    assert not np.array_equal(a, b.astype(np.float64))                       # long bags round in float32: the order matters
    # the witness makes the order matter in every bag of three or more
    for bag in (0, 3, 4):                                                    # 1031, 2 (no witness) and 63 occurrences
        k = slice(off[bag], off[bag + 1])
        rev = href.bag_sum_ref(table, np.array([0, lens[bag]]), feat[k][::-1].copy(), w[k][::-1].copy(), None, np.float32)[0]
        assert np.array_equal(rev[0], b[bag]) == (lens[bag] < 3), bag


# ---- the header, compiled for the host plain and with sanitizers -------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("bag") / ("bag_rule_host_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.run([cxx, "-std=c++17"] + flags + [os.path.join(ROOT, "tests", "host", "bag_rule_host.cpp"), "-o", exe],
                   check=True)
    return exe


def _words(a):
    return " ".join("%08x" % v for v in _bits(a).reshape(-1))


def _ints(a):
    return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1))


def test_the_header_computes_what_the_restatement_computes(host_program, tmp_path):
    rng = np.random.default_rng(4)
    cases = []
    for D in (4, 8, 100, 128):
        nf = 30
        table = href.exact_table(rng, nf, D)
        off, feat, w = href.grid_bags(rng, 8, nf)
        n_bags = off.size - 1
        perm = rng.permutation(n_bags).astype(np.int32)
        rep = rng.integers(1, 8, 12).astype(np.int32)
        rep[:2] = 0                                                          # the longest bag, twice
        bad_rows = np.array([1, -1, 0, n_bags, 3], np.int32)
        bad_feat = feat.copy()
        bad_feat[off[4] + 5] = table.shape[0]                                # one position past the table, in bag 4
        variants = [(rows, weight, ft) for rows in (None, perm, rep, bad_rows) for weight in (None, w)
                    for ft in (feat, bad_feat)]
        if D > 8:                                                            # (the output grows with D: two variants)
            variants = [(perm, w, feat), (rep, None, bad_feat)]
        for rows, weight, ft in variants:
            cases.append(("sum", table, off, ft, weight, rows, None, None, 0.0))
            n = n_bags if rows is None else rows.size
            g = href.exact_table(rng, n, D)[:n]
            valid = (rng.random(n) < 0.7).astype(np.int32)
            valid[0] = 0
            for v in (None, valid):
                cases.append(("expand", table, off, ft, weight, rows, g, v, 0.25))
    # the hand-worked bags
    wit = np.repeat(np.array([2.0 ** 25, 1.0, -2.0 ** 25], np.float32)[:, None], 4, 1)
    cases.append(("sum", wit, np.array([0, 3, 3, 4], np.int64), np.array([0, 1, 2, 1], np.int32), None, None, None, None, 0.0))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for kind, table, off, feat, weight, rows, g, valid, reg in cases:
            n = off.size - 1 if rows is None else rows.size
            head = "%s %d %d %d %d %d %d %d" % (kind, table.shape[0], table.shape[1], feat.size, off.size - 1, n,
                                                weight is not None, rows is not None)
            if kind == "expand":
                head += " %d %s" % (valid is not None, _words(np.float32(reg)))
            parts = [head, _words(table), _ints(off), _ints(feat)]
            parts += [_words(weight)] if weight is not None else []
            parts += [_ints(rows)] if rows is not None else []
            if kind == "expand":
                parts += [_words(g)] + ([_ints(valid)] if valid is not None else [])
            f.write("\n".join(parts) + "\n")
    r = subprocess.run([host_program, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "geometry 128 4 %d" % (1 << 30)
    at, seen_failed = 1, 0
    for kind, table, off, feat, weight, rows, g, valid, reg in cases:
        D = table.shape[1]
        if kind == "sum":
            want, failed = href.bag_sum_ref(table, off, feat, weight, rows, np.float32)
            assert lines[at] == "sum %d %d %d" % (want.shape[0], D, (1 << 30) if failed else 0), lines[at]
            got = np.array([[int(x, 16) for x in l.split()] for l in lines[at + 1:at + 1 + want.shape[0]]], np.uint32)
            assert np.array_equal(got.reshape(want.shape), _bits(want))
            at += 1 + want.shape[0]
        else:
            f, want, oo, failed = href.bag_expand_ref(table, off, feat, weight, rows, g, valid, reg, np.float32)
            M = want.shape[0]
            assert lines[at] == "expand %d %d %d" % (M, D, (1 << 30) if failed else 0), lines[at]
            body = [l.split() for l in lines[at + 1:at + 1 + M]]
            assert [int(l[0]) for l in body] == f.tolist()
            got = np.array([[int(x, 16) for x in l[1:]] for l in body], np.uint32).reshape(M, D)
            assert np.array_equal(got, _bits(want))
            at += 1 + M
        seen_failed += failed
    assert at == len(lines) and seen_failed
    assert lines[-3].split() == ["00000000"] * 4 and lines[-2].split() == ["00000000"] * 4      # the witness, the empty bag
    assert lines[-1].split() == ["3f800000"] * 4


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_the_reference_learns_to_place_withheld_items_from_their_features():
    c = href.planted()
    assert c["new_item"].size * 10 == href.PLANTED["clusters"] * href.PLANTED["items_per"]
    assert not np.isin(c["new_item"], c["item"]).any()
    recall, chance = href.planted_reference_recall(), href.planted_chance()
    print("hybrid planted corpus, fp64 restatement: own withheld recall@%d %.3f, chance %.3f" % (href.PLANTED["k"], recall,
                                                                                                  chance))
    assert recall > 5 * chance

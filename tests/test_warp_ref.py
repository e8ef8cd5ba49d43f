"""CPU: the NumPy reference of the WARP step (tests/_warp_ref.py) -- against BPR's sampler where every unseen candidate
violates, on hand-worked cases for the rank, the weight, the tie and valid = 0, its float32 form against its fp64 form on
the random cases the GPU tests use -- and esr_warp_sample.h, the text the kernel's pieces come from, against it through a
stand-alone host program (tests/host/warp_sample_host.cpp; no HIP, not loaded into Python), also built with the address
and undefined-behaviour sanitizers where the compiler has them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _bpr_ref as bref
import _warp_ref as wref
from conftest import ROOT


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_random_cases_keep_the_undecided_cap_and_float32_agrees_elsewhere():
    for case, r64, r32 in wref.random_cases():
        share = float(r64["undecided"].mean())
        assert share <= wref.UNDECIDED_CAP, (case["name"], share)
        differ = ~wref.same_selection(r32, r64)
        assert not (differ & ~r64["undecided"]).any(), (case["name"], np.flatnonzero(differ))
        assert differ.mean() <= wref.UNDECIDED_CAP and not r64["bad"]
        assert r64["valid"].any() and (r64["trials"] > 1).any(), case["name"]


@pytest.mark.parametrize("B", [1, 65, 257])
def test_where_every_unseen_candidate_violates_the_draw_is_bprs(B):
    rng = np.random.default_rng(21)
    for nu, ni, lengths in ((9, 1001, (1, 2, 63, 64, 65, 1000)), (40, 12, (0, 1, 11, 12)), (2, 1, (1, 0))):
        csr = bref.random_csr(rng, nu, ni, lengths)
        U, Y = wref.random_tables(rng, nu, ni, 8)
        seed, step = (0xC0FFEE << 32) | 99, 2 ** 32 - 1
        r = wref.warp_ref(U, Y, csr, wref.harmonic(ni), seed, step, B, bref.MAX_TRIES, 3e38, 0.0, np.float64)
        u, i, j, valid, _ = bref.sample_ref(*csr, nu, ni, seed, step, 1, B)
        for k, want in zip(("u", "i", "j", "valid"), (u, i, j, valid)):
            assert np.array_equal(r[k], want[0]), (nu, ni, k)
        assert (r["trials"] == r["valid"]).all()                  # the first unseen candidate ends the search


def _one_user(scores, seen, T, margin, weight, seed=1, B=64, D=4):
    """one user x = e_0 and items whose score is their first entry"""
    ni = len(scores)
    U, Y = np.zeros((1, D), np.float32), np.zeros((ni, D), np.float32)
    U[0, 0], Y[:, 0] = 1.0, scores
    csr = bref.csr_of({0: seen}, 1)
    r = wref.warp_ref(U, Y, csr, weight, seed, 0, B, T, margin, 0.25, np.float64)
    cands = (wref.stream_words(seed, 0, B, T + 1)[:, 1:T + 1] * np.uint64(ni)) >> np.uint64(32)
    return r, cands.astype(np.int64), U, Y


def test_hand_worked_rank_weight_tie_and_no_violator():
    ni, T, margin = 10, 6, 0.5
    scores = np.array([2.0, 1.75, 1.5, 1.5, 3.0, 0.0, 0.0, 2.5, 1.0, 1.25])       # item 0 is the seen positive (s_i = 2)
    weight = np.arange(ni + 1, dtype=np.float32) * 0.5                            # w(r) = r / 2
    r, cands, U, Y = _one_user(scores, [0], T, margin, weight)
    violates = {1: True, 2: False, 3: False, 4: True, 5: False, 6: False, 7: True, 8: False, 9: False}   # d < 1 / 2; 2, 3 tie
    seen_classes = set()
    for t in range(64):
        N, got = 0, None
        for c in cands[t]:
            if c == 0:
                continue                                                        # seen: skipped, not counted
            N += 1
            if violates[int(c)]:
                got = int(c)
                break
        assert r["trials"][t] == N and r["u"][t] == 0 and r["i"][t] == 0
        if got is None:
            assert r["valid"][t] == 0 and r["j"][t] == cands[t][-1] and r["loss_t"][t] == 0 and r["d"][t] == 0
            assert not r["grads"][[t, 64 + t, 128 + t]].any()
            seen_classes.add("none")
            continue
        rank = max(1, (ni - 1) // N)
        d = 2.0 - scores[got]
        assert r["valid"][t] == 1 and r["j"][t] == got and r["d"][t] == d
        assert r["loss_t"][t] == weight[rank] * (margin - d)
        w = float(weight[rank])
        assert np.array_equal(r["grads"][t], 0.25 * U[0] - w * (Y[0] - Y[got]))
        assert np.array_equal(r["grads"][64 + t], 0.25 * Y[0] - w * U[0])
        assert np.array_equal(r["grads"][128 + t], 0.25 * Y[got] + w * U[0])
        seen_classes.add(("rank", rank))
    assert "none" in seen_classes and {("rank", 9), ("rank", 4), ("rank", 3)} <= seen_classes
    # a tie alone never violates; one 2^-6 below does
    tie, _, _, _ = _one_user(np.array([2.0] + [1.5] * 9), [0], T, margin, weight)
    assert not tie["valid"].any() and (tie["trials"] > 0).all()
    below, _, _, _ = _one_user(np.array([2.0] + [1.5 + 2.0 ** -6] * 9), [0], T, margin, weight)
    assert (below["valid"] == (below["trials"] > 0)).all() and (below["d"][below["valid"] == 1] == 0.5 - 2.0 ** -6).all()
    # a user who has seen everything: no trial, no triple
    full, cands, _, _ = _one_user(scores, list(range(ni)), T, margin, weight)
    assert not full["valid"].any() and not full["trials"].any() and np.array_equal(full["j"], cands[:, -1])
    # a position outside the table: zeros and the flag
    U, Y = np.ones((1, 4), np.float32), np.ones((3, 4), np.float32)
    off = wref.warp_ref(U, Y, (np.array([0, 1]), np.array([0]), np.array([7])), weight[:4], 1, 0, 8, 4, 0.5, 0.25, np.float64)
    assert off["bad"] and not off["valid"].any() and not off["trials"].any() and not off["j"].any() and not off["grads"].any()


def test_the_cases_cover_every_class_of_search():
    """a later change of seeds must not empty a class silently"""
    classes = set()
    for case, r in wref.exact_cases():
        T = case["T"]
        for valid, n in set(zip(r["valid"].tolist(), r["trials"].tolist())):
            classes.add(("trials", n))
            if n == T:
                classes.add(("trials", "T"))
            if not valid:
                classes.add(("dropped", 0 if n == 0 else ("T" if n == T else "between")))
    assert {("trials", 1), ("trials", 4), ("trials", 5), ("trials", "T"), ("trials", 255), ("dropped", 0),
            ("dropped", "T")} <= classes, sorted(map(str, classes))
    ties = next(r for c, r in wref.exact_cases() if c["name"] == "ties")
    assert ties["valid"].all() and (ties["trials"] > 1).any()         # ties were walked past


def test_chosen_slots_equal_the_same_rows_of_the_whole_step():
    """warp_ref(slots=...) is the whole restatement's rows at those slots, for every key: an exact case, a random one in
    both dtypes, slots out of order with a repeat, and the empty choice"""
    exact = next((c, r) for c, r in wref.exact_cases() if c["name"] == "grid-D100-B257-T5")
    rand = wref.random_cases()[1]                                    # D 64, B 1024, T 32
    for case, full, dtype in (exact + (np.float64,), (rand[0], rand[1], np.float64), (rand[0], rand[2], np.float32)):
        B = case["B"]
        for slots in (np.array([B - 1, 0, 63, 64, 65, 0, B // 2]), np.arange(B - 7, B), np.arange(B), np.zeros(0, np.int64)):
            part = wref.warp_ref(case["user"], case["item"], case["csr"], case["weight"], case["seed"], case["step"], B,
                                 case["T"], case["margin"], case["reg"], dtype, slots=slots)
            assert set(part) == set(full)
            for k in wref.IDS + ("s_i", "d", "loss_t", "undecided"):
                assert part[k].dtype == full[k].dtype and np.array_equal(part[k], full[k][slots]), (case["name"], k)
            assert part["grads"].shape == (3 * slots.size, case["user"].shape[1]) and part["grads"].dtype == full["grads"].dtype
            for third in range(3):
                assert np.array_equal(part["grads"][third * slots.size:(third + 1) * slots.size],
                                      full["grads"][third * B + slots]), (case["name"], third)
            assert part["bad"] is False and full["bad"] is False
        words = wref.stream_words(case["seed"], case["step"], B, case["T"] + 1)
        two = wref.stream_words(case["seed"], case["step"], B, case["T"] + 1, slots=[B - 1, 3])
        assert np.array_equal(two, words[[B - 1, 3]])
    with pytest.raises(AssertionError):
        wref.stream_words(1, 0, 8, 4, slots=[8])                     # a slot number is below B


def test_rank_weight_tables():
    h = wref.harmonic(5)
    assert h.dtype == np.float32 and h[0] == 0 and h[1] == 1 and h[2] == 1.5 and h[5] == np.float32(137.0 / 60.0)


# ---- the header, compiled for the host -----------------------------------------------------------------------------------
def _compile(tmp, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags +
                       [os.path.join(ROOT, "tests", "host", "warp_sample_host.cpp"), "-o", exe, "-lm"], capture_output=True,
                       text=True)
    return exe if r.returncode == 0 else None, r.stderr


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    """the host program's answers to every shared case, from the plain build; the sanitised build, where the compiler has
    the sanitizers, must print the same text"""
    tmp = tmp_path_factory.mktemp("warp")
    plain, err = _compile(tmp, "warp_sample_host", [])
    assert plain is not None, err[-2000:]
    cases = [c for c, _ in wref.exact_cases()] + [c for c, _, _ in wref.random_cases()]
    path = tmp / "cases.txt"
    bits = lambda a: " ".join(str(int(v)) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))   # noqa: E731
    with open(path, "w") as f:
        for c in cases:
            off, upos, ipos = c["csr"]
            nu, D = c["user"].shape
            f.write("%d %d %d %d %d %d %d %d %s %s\n" % (nu, c["item"].shape[0], upos.size, D, c["seed"], c["step"], c["B"],
                                                         c["T"], bits(c["margin"]), bits(c["reg"])))
            for a in (off, upos, ipos):
                f.write(" ".join(str(int(v)) for v in a) + "\n")
            for a in (c["weight"], c["user"], c["item"]):
                f.write(bits(a) + "\n")
    r = subprocess.run([plain, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    sanitised, _ = _compile(tmp, "warp_sample_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if sanitised is not None:
        s = subprocess.run([sanitised, str(path)], capture_output=True, text=True)
        assert s.returncode == 0, s.stderr[-4000:]
        assert s.stdout == r.stdout
    lines = r.stdout.splitlines()
    assert lines[0] == "max_trials %d" % wref.MAX_TRIALS
    out, at = {}, 1
    for c in cases:
        assert lines[at] == "case %d" % c["B"]
        rows = np.array([l.split() for l in lines[at + 1:at + 1 + c["B"]]], dtype=np.int64)
        at += 1 + c["B"]
        got = {k: rows[:, n].astype(np.int32) for n, k in enumerate(wref.IDS)}
        got["s_i"] = rows[:, 5].astype(np.uint32).view(np.float32)
        got["d"] = rows[:, 6].astype(np.uint32).view(np.float32)
        out[c["name"]] = got
    assert at == len(lines)
    return out


def test_the_header_equals_the_restatement_bit_for_bit_on_exact_tables(host_run):
    for case, r in wref.exact_cases():
        got = host_run[case["name"]]
        for k in wref.IDS:
            assert np.array_equal(got[k], r[k]), (case["name"], k)
        assert np.array_equal(got["s_i"], r["s_i"].astype(np.float32)), case["name"]
        assert np.array_equal(got["d"], r["d"].astype(np.float32)), case["name"]


def test_the_header_selects_what_the_restatement_selects_on_random_tables(host_run):
    ulp = float(np.finfo(np.float32).eps)
    for case, r64, _ in wref.random_cases():
        got = host_run[case["name"]]
        same = wref.same_selection(got, r64)
        assert not (~same & ~r64["undecided"]).any(), (case["name"], np.flatnonzero(~same))
        # s_i and d within a few ulp of the terms' size: D <= 128 terms, each rounded once (fmaf) and summed in a tree
        x, yi, yj = (np.abs(a).astype(np.float64) for a in (case["user"][r64["u"]], case["item"][r64["i"]], case["item"][r64["j"]]))
        size_i, size_j = (x * yi).sum(1), (x * yj).sum(1)
        assert (np.abs(got["s_i"] - r64["s_i"]) <= 4 * ulp * size_i).all(), case["name"]
        ok = same & (r64["valid"] == 1)
        assert (np.abs(got["d"] - r64["d"])[ok] <= 4 * ulp * (size_i + size_j)[ok]).all(), case["name"]
        assert not got["d"][r64["valid"] == 0][same[r64["valid"] == 0]].any()


# ---- learning ----------------------------------------------------------------------------------------------------------------
def planted_start():
    """the factors factorization.WARP draws on the planted corpus: randn * rank^-1/2 from the seeded CPU generator"""
    import torch
    nu, ni, rank = wref.PLANTED["nu"], wref.PLANTED["ni"], wref.PLANTED["rank"]
    gen = torch.Generator(device="cpu").manual_seed(wref.PLANTED["seed"])
    U = (torch.randn(nu, rank, generator=gen) * float(rank) ** -0.5).numpy()
    return U, (torch.randn(ni, rank, generator=gen) * float(rank) ** -0.5).numpy()


def test_the_reference_learns_the_planted_communities_and_its_negatives_get_harder():
    before, after, trials, losses = wref.planted_run(*planted_start())
    print("planted WARP reference: auc %.4f -> %.4f, mean trials %.3f -> %.3f" % (before, after, trials[0], trials[-1]))
    assert np.isfinite(losses).all() and len(trials) == 60
    assert after > before and trials[-1] > trials[0]
    assert abs(after - 0.8789) <= 5e-4 and abs(before - 0.5430) <= 5e-4      # the values _warp_ref's docstring records

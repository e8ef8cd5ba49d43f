"""The Spotify two-tower step (esr_spotify.hip) across its kernel dispatch, widths and sizes, against the fp64 oracle.

Which kernels a playlist of n context, m next and o negative rows of width 2F runs is decided by two formulas
(R = n + m + o, S = m + o):

  row gradient   spotify_rowgrad_kernel<NCH, STAGED>: NCH = 1 / 2 / 4 for ceil(2F / 64) = 1 / 2 / 3 or 4;
                 STAGED iff R * 2F * 4 <= 64 KiB, i.e. R * 2F <= 16384          (esr_spotify.hip: rg_lds / staged in sp_fwd_bwd)
                 and ESR_SPOTIFY_ROWGRAD != global; its staging copy is float4 iff 2F % 4 == 0
  affinity       spotify_affinity_lds_kernel iff (R (2F + 1) + S n) * 4 + 1024 <= 150 KiB, i.e. R (2F + 1) + S n <= 38144
                 (esr_spotify.hip: sp_aff_lds_bytes / sp_affinity_in_lds) and ESR_SPOTIFY_AFFINITY != global; else
                 spotify_affinity_kernel, whose dot products are float4 iff 2F % 4 == 0

staged() / aff_lds() below restate them; every case names the forms it expects and test_cases_select_every_form checks
the names against the formulas and that no (affinity form, NCH, STAGED, 2F % 4) combination is left unvisited.  Every
case runs under the default dispatch and with either form forced to `global`; the table lists what the DEFAULT picks:

  case               2F   NCH  2F%4  R     staged  affinity   what else it is there for
  f4_n1              8    1    0     12    yes     lds        n = 1, m % 4 = 1, o % 4 = 2
  f5_n2              10   1    2     18    yes     lds        scalar staging copy, n = 2, m % 4 = 3, o % 4 = 1
  f24                48   1    0     87    yes     lds        a width below one chunk, m % 4 = 2
  f32                64   1    0     90    yes     lds        the reference's width
  f33                66   2    2     90    yes     lds        a two-chunk width that is no multiple of 4, o % 4 = 3
  f64_n31            128  2    0     119   yes     lds        n = 31 (n % 4 = 3), S = 88 (no multiple of 64), S n > 1024
  f80                160  4    0     99    yes     lds        the 3-chunk width (last chunk short)
  f81                162  4    2     99    yes     lds        3 chunks, scalar copy
  f128_n32           256  4    0     63    yes     lds        the caps n = 32 and 2F = 256
  rg_f32_256 / 257   64   1    0     ...   yes/no  lds        16384 / 64  = 256
  rg_f64_128 / 129   128  2    0     ...   yes/no  lds        16384 / 128 = 128
  rg_f128_64 / 65    256  4    0     ...   yes/no  lds        16384 / 256 = 64
  rg_f80_102 / 103   160  4    0     ...   yes/no  lds        16384 / 160 = 102.4
  rg_f33_248 / 249   66   2    2     ...   yes/no  lds        16384 / 66  = 248.2
  aff_f32_545 / 546  64   1    0     ...   no      lds/global 70 R - 25 <= 38144: R <= 545.2
  aff_f128_135 / 136 256  4    0     ...   no      lds/global 289 R - 1024 <= 38144: R <= 135.5 (n = 32)
  aff_f33_530 / 531  66   2    2     ...   no      lds/global 72 R - 25 <= 38144: R <= 530.1: the scalar global branch by size
  aff_f81_227 / 228  162  4    2     ...   no      lds/global 168 R - 25 <= 38144: R <= 227.2
  big_f4             8    1    0     1105  yes     lds        S = 1100 > 1024: a second trip of the 1024-thread strides
  conc_f32           64   1    0     199   yes     lds        every negative's best context is ONE row: 64 weights per ballot
                                                              chunk for it, none for the other context rows
  (forced: ROWGRAD=global gives <NCH, unstaged> for every row above, AFFINITY=global the global kernel in both of its
  branches -- together with the defaults: {lds, global} x {1, 2, 4} x {staged, unstaged} x {2F % 4 = 0, 2})

The bar is the project's 1e-5 relative against the fp64 oracle.  The loss has hard decisions (row max, min / max, relus,
the kinks of up to 10^6 self-affinity pairs); oracle() finds the decisions an f32 implementation may legitimately take
the other way -- a dot product a.b within 2 * 2F * 2^-24 * |a||b| of what it is compared with: twice the a-priori bound of
an f32 fma chain of length 2F -- asserts that a case has none except a few self-affinity pairs, and widens the bar of
exactly the two rows such a pair touches by what the pair contributes.  Nothing here is measured on a GPU."""
import functools
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_golden, rel_err
from oracle import spotify as o_sp

gpu = pytest.mark.gpu
TOL = 1e-5                    # (tests/test_gpu_spotify.py)
F64 = np.float64
A = o_sp.MAX_ALBUMS           # the oracle hashes with it: the album table has exactly this many rows
N_ART = 3000
U24 = 2.0 ** -24              # unit roundoff of f32


def staged(n, m, o, F):
    return (n + m + o) * 2 * F * 4 <= 64 * 1024


def aff_lds(n, m, o, F):
    return ((n + m + o) * (2 * F + 1) + (m + o) * n) * 4 + 1024 <= 150 * 1024


def nch(F):
    return {1: 1, 2: 2, 3: 4, 4: 4}[-(-2 * F // 64)]


Case = namedtuple("Case", "name n m o F reg aff staged seed conc")


def _c(name, n, m, o, F, reg, aff, stg, seed, conc=False):
    return Case(name, n, m, o, F, reg, aff, stg, seed, conc)


# `aff` / `staged`: what the default dispatch picks (checked against the formulas); seeds: the first for which oracle()'s
# conditions hold (found by running the CPU test below; a case whose conditions fail FAILS, it is never left out)
CASES = [
    _c("f4_n1", 1, 5, 6, 4, 2.8, "lds", True, 0),
    _c("f5_n2", 2, 7, 9, 5, 2.8, "lds", True, 0),
    _c("f24", 5, 18, 64, 24, 2.8, "lds", True, 0),
    _c("f32", 5, 21, 64, 32, 2.8, "lds", True, 0),
    _c("f33", 5, 22, 63, 33, 10.0, "lds", True, 0),
    _c("f64_n31", 31, 23, 65, 64, 2.8, "lds", True, 0),
    _c("f80", 5, 30, 64, 80, 2.8, "lds", True, 0),
    _c("f81", 5, 30, 64, 81, 2.8, "lds", True, 0),
    _c("f128_n32", 32, 10, 21, 128, 2.8, "lds", True, 0),
    _c("rg_f32_256", 5, 187, 64, 32, 2.8, "lds", True, 0),
    _c("rg_f32_257", 5, 188, 64, 32, 2.8, "lds", False, 0),
    _c("rg_f64_128", 5, 59, 64, 64, 2.8, "lds", True, 0),
    _c("rg_f64_129", 5, 60, 64, 64, 2.8, "lds", False, 0),
    _c("rg_f128_64", 2, 32, 30, 128, 2.8, "lds", True, 0),
    _c("rg_f128_65", 2, 33, 30, 128, 2.8, "lds", False, 0),
    _c("rg_f80_102", 5, 33, 64, 80, 2.8, "lds", True, 3),
    _c("rg_f80_103", 5, 34, 64, 80, 2.8, "lds", False, 0),
    _c("rg_f33_248", 5, 179, 64, 33, 2.8, "lds", True, 0),
    _c("rg_f33_249", 5, 180, 64, 33, 2.8, "lds", False, 0),
    _c("aff_f32_545", 5, 476, 64, 32, 2.8, "lds", False, 0),
    _c("aff_f32_546", 5, 477, 64, 32, 2.8, "global", False, 0),
    _c("aff_f128_135", 32, 39, 64, 128, 2.8, "lds", False, 0),
    _c("aff_f128_136", 32, 40, 64, 128, 2.8, "global", False, 1),
    _c("aff_f33_530", 5, 461, 64, 33, 2.8, "lds", False, 0),
    _c("aff_f33_531", 5, 462, 64, 33, 2.8, "global", False, 0),
    _c("aff_f81_227", 5, 158, 64, 81, 2.8, "lds", False, 0),
    _c("aff_f81_228", 5, 159, 64, 81, 2.8, "global", False, 0),
    _c("big_f4", 5, 1030, 70, 4, 2.8, "lds", True, 0),
    _c("conc_f32", 5, 64, 130, 32, 10.0, "lds", True, 0, conc=True),
]
IDS = [c.name for c in CASES]


# ------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def tables(F):
    """album [100000, F] and artist [3000, F] tables, rows scaled by 2 / sqrt(F) (|row of E|^2 ~ 8)"""
    rng = np.random.default_rng(1000 + F)
    at = (rng.standard_normal((A, F)) * (2.0 / np.sqrt(F))).astype(np.float32)
    rt = (rng.standard_normal((N_ART, F)) * (2.0 / np.sqrt(F))).astype(np.float32)
    return at, rt


def plant(album, artist, n, m):
    """What every playlist here contains (m >= 4): a duplicated context row (n >= 2), a duplicated next row, a next row
    equal to a context row, and one album-id pair (a, a + A) -- one table row, two raw ids -- split between the context
    and the next group, with different artists: the embedding halves and the update share the row, the `in context`
    boost compares raw ids and must not fire."""
    assert m >= 4
    cc = n // 2 if n >= 3 else 0
    album[cc] %= A
    if n >= 2:
        album[n - 1], artist[n - 1] = album[0], artist[0]
    album[n + 1], artist[n + 1] = album[n], artist[n]
    album[n + 2], artist[n + 2] = album[0], artist[0]
    album[n + 3], artist[n + 3] = album[cc] + A, (artist[cc] + 1) % N_ART
    return album, artist


def inputs_of(case):
    """(album_table, artist_table, album ids [R], artist ids [R]) of a case, f32 / int32"""
    at, rt = tables(case.F)
    n, m, o = case.n, case.m, case.o
    rng = np.random.default_rng(case.seed * 1000 + sum(map(ord, case.name)))
    album = rng.integers(0, 4 * A, n + m + o)
    artist = rng.integers(0, N_ART, n + m + o)
    plant(album, artist, n, m)
    if case.conc:
        # every negative is by context row 0's artist, whose table row is three times as long: |artist half|^2 ~ 36
        # outweighs any album half (~ 4 +- 1), so context row 0 (and its duplicate) is every negative's row maximum
        artist[n + m:] = artist[0]
        rt = rt.copy()
        rt[artist[0]] *= 3.0
    return at, rt, album.astype(np.int32), artist.astype(np.int32)


def batch_of(album, artist, n, m):
    return {"album_context": album[:n], "artist_context": artist[:n], "next_album": album[n:n + m],
            "next_artist": artist[n:n + m], "neg_album": album[n + m:], "neg_artist": artist[n + m:]}


# -------------------------------------------------------------------------------------------------- comparator
def oracle(at64, rt64, album, artist, n, m, o, reg, what, max_pair_frac=1e-3):
    """The fp64 result and its ambiguous decisions.  A decision that compares a dot product a.b (of 2F terms) with a
    threshold or another dot product is ambiguous when the gap is at most 2 * 2F * 2^-24 * |a||b| (the sum of the two
    bounds when both sides are dot products); exact ties of identical rows are not -- they tie in every precision.
    ASSERTS: no ambiguous row-max, min / max, head-relu or norm decision; ambiguous self-affinity pairs in at most
    max_pair_frac of a group's pairs.  slack[r]: what the ambiguous pairs of row r may contribute to its gradient,
    (2 / Rg^2) |E_a|_inf each -- the only widening of the bar there is."""
    F = at64.shape[1]
    R, S = n + m + o, m + o
    x = batch_of(album, artist, n, m)
    loss, aid, arows, rid, rrows = o_sp.loss_and_row_grads(at64, rt64, x, reg)
    E = o_sp.get_embeddings(at64, rt64, album, artist)
    nrm = np.sqrt((E * E).sum(axis=1))
    u = 2.0 * (2 * F) * U24
    same_row = (aid[:, None] == aid[None, :]) & (rid[:, None] == rid[None, :])          # identical embeddings
    al64 = np.asarray(album, np.int64)
    same_occ = (al64[:, None] == al64[None, :]) & (rid[:, None] == rid[None, :])        # ... and identical boosts
    # ---- row max over the contexts
    raw = E[n:] @ E[:n].T
    bnd = u * nrm[n:, None] * nrm[None, :n]
    ar = np.arange(S)
    best = raw.argmax(axis=1)
    top = raw[ar, best]
    amb = ((top[:, None] - raw) <= bnd[ar, best][:, None] + bnd) & ~same_row[best][:, :n]
    assert not amb.any(), "%s: ambiguous row max in scored rows %s" % (what, np.nonzero(amb.any(axis=1))[0][:8])
    # ---- min over the positives, max over the negatives
    aff = top + o_sp.BOOST * np.isin(album[n:], album[:n]) + o_sp.BOOST * np.isin(artist[n:], artist[:n])
    affb = bnd[ar, best] + 4 * U24 * (np.abs(top) + 2 * o_sp.BOOST)
    for lo, hi, sign, name in ((0, m, 1.0, "min of the positives"), (m, S, -1.0, "max of the negatives")):
        v = sign * aff[lo:hi]
        k = int(v.argmin())
        amb = ((v - v[k]) <= affb[lo:hi] + affb[lo + k]) & ~same_occ[n + lo + k, n + lo:n + hi]
        assert not amb.any(), "%s: ambiguous %s" % (what, name)
    # ---- the two head relus
    pos, neg = aff[:m], aff[m:]
    mt_arg = 1.0 + neg.mean() - pos.mean()
    et_arg = 1.0 + neg.max() - pos.min()
    mt_b = affb[:m].mean() + affb[m:].mean() + 4 * U24 * (1.0 + abs(neg.mean()) + abs(pos.mean()))
    et_b = affb[m + int(neg.argmax())] + affb[int(pos.argmin())] + 4 * U24 * (1.0 + abs(neg.max()) + abs(pos.min()))
    assert abs(mt_arg) > mt_b and abs(et_arg) > et_b, "%s: ambiguous head relu (%g, %g)" % (what, mt_arg, et_arg)
    # ---- the norm term: |E_b| = sqrt of a chain of 2F squares against the regularization
    amb = np.abs(nrm - reg) <= (u + 2 * U24) * nrm
    assert not amb.any(), "%s: ambiguous norm decision in rows %s" % (what, np.nonzero(amb)[0][:8])
    # ---- the self-affinity kinks: s < 0.5 (pull: context, next), s > 0 (push: negatives)
    slack = np.zeros(R)
    pairs = 0
    for g0, Rg, thr in ((0, n, 0.5), (n, m, 0.5), (n + m, o, 0.0)):
        G = E[g0:g0 + Rg]
        amb = np.abs(G @ G.T - thr) <= u * nrm[g0:g0 + Rg, None] * nrm[None, g0:g0 + Rg]
        assert amb.sum() <= max_pair_frac * Rg * Rg, \
            "%s: %d of %d^2 self-affinity pairs are ambiguous" % (what, amb.sum(), Rg)
        slack[g0:g0 + Rg] += (amb * np.abs(G).max(axis=1)[:, None]).sum(axis=0) * (2.0 / (Rg * Rg))
        pairs += int(amb.sum())
    return SimpleNamespace(loss=loss, aid=aid, arows=arows, rid=rid, rrows=rrows, slack=slack, pairs=pairs, x=x)


def compare(ora, loss, ga, gr, what):
    """loss and both gradient blocks within 1e-5 of the oracle (max |a - b| / max |b| per block, as rel_err); a row that
    an ambiguous self-affinity pair touches may be off by that pair's contribution on top"""
    assert abs(float(loss) - ora.loss) <= TOL * abs(ora.loss), (what, float(loss), ora.loss)
    for got, exp, blk in ((ga, ora.arows, "album"), (gr, ora.rrows, "artist")):
        if not ora.slack.any():
            assert rel_err(got, exp) <= TOL, (what, blk)
            continue
        err = np.abs(np.asarray(got, F64) - exp).max(axis=1)
        allowed = TOL * np.abs(exp).max() + ora.slack
        bad = np.nonzero(err > allowed)[0]
        assert bad.size == 0, (what, blk, bad[:8], err[bad[:8]], allowed[bad[:8]])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_f32_oracle_passes_the_comparator(case):
    """CPU: the oracle evaluated in f32 is inside the bar for exactly the inputs the GPU tests use -- a correct f32
    implementation can pass, and every case meets the comparator's conditions (none is left out)."""
    at, rt, album, artist = inputs_of(case)
    ora = oracle(at.astype(F64), rt.astype(F64), album, artist, case.n, case.m, case.o, case.reg, case.name)
    x = batch_of(album, artist, case.n, case.m)
    loss, aid, arows, rid, rrows = o_sp.loss_and_row_grads(at, rt, x, np.float32(case.reg), dtype=np.float32)
    assert np.array_equal(aid, ora.aid) and np.array_equal(rid, ora.rid)
    compare(ora, loss, arows, rrows, case.name + " in f32")
    # what every case plants
    n, m = case.n, case.m
    assert album[n + 3] == album[n // 2 if n >= 3 else 0] + A and ora.aid[n + 3] == ora.aid[n // 2 if n >= 3 else 0]
    assert (album[n + 2], artist[n + 2]) == (album[0], artist[0]) and (album[n + 1], artist[n + 1]) == (album[n], artist[n])
    assert n == 1 or (album[n - 1], artist[n - 1]) == (album[0], artist[0])


def test_cases_select_every_form():
    """CPU: each case's named forms are what the two formulas give, both sides of every edge are one row apart, and the
    cases with their forced variants visit every (affinity form, NCH, STAGED, 2F % 4) combination."""
    seen = set()
    for c in CASES:
        assert staged(c.n, c.m, c.o, c.F) == c.staged, c.name
        assert ("lds" if aff_lds(c.n, c.m, c.o, c.F) else "global") == c.aff, c.name
        assert 1 <= c.n <= 32 and 2 * c.F <= 256
        for aff in {c.aff, "global"}:
            for stg in {c.staged, False}:
                seen.add((aff, nch(c.F), stg, 2 * c.F % 4))
    assert seen == {(a, k, s, p) for a in ("lds", "global") for k in (1, 2, 4) for s in (True, False) for p in (0, 2)}
    by = {c.name: c for c in CASES}
    for lo, hi in (("rg_f32_256", "rg_f32_257"), ("rg_f64_128", "rg_f64_129"), ("rg_f128_64", "rg_f128_65"),
                   ("rg_f80_102", "rg_f80_103"), ("rg_f33_248", "rg_f33_249")):
        a, b = by[lo], by[hi]
        assert (a.n, a.m + 1, a.o, a.F) == (b.n, b.m, b.o, b.F) and a.staged and not b.staged
    for lo, hi in (("aff_f32_545", "aff_f32_546"), ("aff_f128_135", "aff_f128_136"), ("aff_f33_530", "aff_f33_531"),
                   ("aff_f81_227", "aff_f81_228")):
        a, b = by[lo], by[hi]
        assert (a.n, a.m + 1, a.o, a.F) == (b.n, b.m, b.o, b.F) and a.aff == "lds" and b.aff == "global"
    assert {c.n for c in CASES} >= {1, 2, 5, 31, 32} and {c.F for c in CASES} >= {4, 5, 24, 32, 33, 64, 80, 128}
    for grp in ("n", "m", "o"):
        assert {getattr(c, grp) % 4 for c in CASES} >= {1, 2, 3}, grp
    assert any((c.m + c.o) % 64 and (c.m + c.o) * c.n > 1024 for c in CASES)
    assert any(c.m + c.o > 1024 and c.aff == "lds" for c in CASES)


# ---------------------------------------------------------------------------------- fwd_bwd / forward on the GPU
def T(x, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


_DEV = {}


def dev_tables(case, rt, dev):
    """the tables of a width on the device (one upload per width; the concentrated case has its own artist table)"""
    if case.F not in _DEV:
        _DEV[case.F] = tuple(T(t, dev) for t in tables(case.F))
    at_d, rt_d = _DEV[case.F]
    return at_d, (T(rt, dev) if case.conc else rt_d)


def set_forms(monkeypatch, aff, rg):
    """'default': the variable unset (the library reads both per call)"""
    for var, val in (("ESR_SPOTIFY_AFFINITY", aff), ("ESR_SPOTIFY_ROWGRAD", rg)):
        if val == "default":
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fwd_bwd_vs_oracle_over_the_dispatch_matrix(dev, case, monkeypatch):
    """esr_spotify_fwd_bwd in all four (affinity, row gradient) forms against the oracle: hashed rows bit-equal, loss and
    gradient blocks through the comparator.  Between forms: partner rows from LDS or from global memory are the same
    operations on the same values -- bit-equal; the two affinity kernels agree to the 1e-6 of
    test_affinity_from_lds_equals_affinity_from_global_memory (their fp64 loss sums associate differently)."""
    import torch
    from esrecsys_amd import ops
    at, rt, album, artist = inputs_of(case)
    n, m, o = case.n, case.m, case.o
    ora = oracle(at.astype(F64), rt.astype(F64), album, artist, n, m, o, case.reg, case.name)
    at_d, rt_d = dev_tables(case, rt, dev)
    al, ar = T(album, dev), T(artist, dev)
    got = {}
    for aff in ("default", "global"):
        for rg in ("default", "global"):
            set_forms(monkeypatch, aff, rg)
            loss, rows, ga, gr = ops.spotify_fwd_bwd(at_d, rt_d, al, ar, n, m, o, case.reg)
            what = "%s affinity=%s rowgrad=%s" % (case.name, aff, rg)
            assert np.array_equal(N(rows), ora.aid), what
            compare(ora, float(loss), N(ga), N(gr), what)
            got[aff, rg] = (loss, ga, gr)
    for aff in ("default", "global"):
        for x, y in zip(got[aff, "default"], got[aff, "global"]):
            assert torch.equal(x, y), (case.name, aff)
    (la, gaa, gra), (lb, gab, grb) = got["default", "default"], got["global", "default"]
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))
    assert float((gaa - gab).abs().max()) <= 1e-6 * float(gab.abs().max())
    assert float((gra - grb).abs().max()) <= 1e-6 * float(grb.abs().max())


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_vs_oracle_over_the_dispatch_matrix(dev, case, monkeypatch):
    """esr_spotify_forward's six outputs (the self-affinity matrices with their row flip among them) with either
    affinity kernel"""
    from esrecsys_amd import ops
    at, rt, album, artist = inputs_of(case)
    n, m, o = case.n, case.m, case.o
    exp = o_sp.forward(at.astype(F64), rt.astype(F64), batch_of(album, artist, n, m))
    at_d, rt_d = dev_tables(case, rt, dev)
    al, ar = T(album, dev), T(artist, dev)
    for aff in ("default", "global"):
        set_forms(monkeypatch, aff, "default")
        out = ops.spotify_forward(at_d, rt_d, al, ar, n, m, o)
        assert [tuple(t.shape) for t in out] == [(m,), (o,), (n, n), (m, m), (o, o), (n + m + o,)]
        for got, e, key in zip(out, exp, ("pos", "neg", "ctx_self", "next_self", "neg_self", "l2")):
            assert rel_err(N(got), e) <= TOL, (case.name, aff, key)


# ------------------------------------------------------------------------------------------------ the train step
# A flipped near-kink decision would move a table row by lr * 2 / Rg^2 -- far above 1e-5 -- and every later step with it,
# so a stream must have NO ambiguous decision at all (oracle(max_pair_frac=0) at every step).  An f32 chain of 2F terms
# leaves a window of 4 (2F)^1.5 2^-24 standard deviations around a kink: 5e-6 at 2F = 8, 1e-3 at 2F = 256.  The narrow
# widths therefore run on the tables of the dispatch matrix; the wide ones on rows 0.15 times as long (|E_a||E_b| ~ 0.2:
# every pull pair is far below 0.5) with a handful of negatives (the push kink at 0 has no such margin), and leave the
# kinks to the fwd_bwd matrix above, which runs the same row-gradient kernels.
TCase = namedtuple("TCase", "name F n m o scale reg seed")
TRAIN = [
    TCase("f4_n1_handful", 4, 1, 5, 6, 1.0, 2.8, 0),
    TCase("f5", 5, 5, 40, 64, 1.0, 2.8, 0),
    TCase("f24_unstaged", 24, 5, 330, 8, 0.15, 0.42, 1),         # R = 343 > 16384 / 48
    TCase("f33_n32", 33, 32, 20, 7, 0.15, 0.42, 0),
    TCase("f64_unstaged", 64, 5, 125, 6, 0.15, 0.42, 0),         # R = 136 > 128
    TCase("f128_n32_unstaged", 128, 32, 30, 5, 0.15, 0.42, 1),   # R = 67 > 64
]
TIDS = [t.name for t in TRAIN]
# step numbers advance by these: the resident row (occurrence 0 of every playlist) is read with gaps of
# increment - 1 = 0, 1, 64 (kLazyExact, esr_common.h: the last gap applied step by step) and 65 (the closed form)
INCREMENTS = (1, 1, 2, 65, 66, 1, 1, 2, 1, 1, 1, 1)
LR, MOM = 0.05, 0.9


def train_start(tc):
    at, rt = tables(tc.F)
    rng = np.random.default_rng(77 + tc.F)
    s = np.float32(tc.scale)
    return [at * s, (rng.standard_normal(at.shape) * 0.01 * tc.scale).astype(np.float32),
            rt * s, (rng.standard_normal(rt.shape) * 0.01 * tc.scale).astype(np.float32)]


def train_stream(tc):
    """[(step number, album ids, artist ids)]: random playlists, every third one by 30 hot artists (rows that repeat
    inside a playlist), each with plant()'s duplicates and hash collision and with one resident track at the front"""
    rng = np.random.default_rng(tc.seed * 1000 + sum(map(ord, tc.name)))
    R = tc.n + tc.m + tc.o
    res_album, res_artist = int(rng.integers(0, A)), int(rng.integers(0, N_ART))
    step, out = 0, []
    for it, inc in enumerate(INCREMENTS):
        step += inc
        album = rng.integers(0, 4 * A, R)
        artist = rng.integers(0, 30 if it % 3 == 1 else N_ART, R)
        album[0], artist[0] = res_album, res_artist
        plant(album, artist, tc.n, tc.m)
        out.append((step, album.astype(np.int32), artist.astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def train_oracle(tc):
    """The dense fp64 run: o_sp.dense_grads + o_sp.sgd_momentum_update at every step of the stream; a step number nobody
    trains on is a step with a zero gradient (trace = momentum * trace; p -= lr * trace, on every row).
    -> (losses, album table, album trace, artist table, artist trace)"""
    at, ta, rt, tr = [t.astype(F64) for t in train_start(tc)]
    losses, prev = [], 0
    for step, album, artist in train_stream(tc):
        for _ in range(step - prev - 1):
            ta *= MOM
            at -= LR * ta
            tr *= MOM
            rt -= LR * tr
        what = "%s step %d" % (tc.name, step)
        ora = oracle(at, rt, album, artist, tc.n, tc.m, tc.o, tc.reg, what, max_pair_frac=0.0)
        el, ga, gr = o_sp.dense_grads(at, rt, ora.x, tc.reg)
        assert el == ora.loss
        at, ta = o_sp.sgd_momentum_update(at, ta, ga, LR, MOM, F64)
        rt, tr = o_sp.sgd_momentum_update(rt, tr, gr, LR, MOM, F64)
        losses.append(el)
        prev = step
    return losses, at, ta, rt, tr


@pytest.mark.parametrize("tc", TRAIN, ids=TIDS)
def test_train_streams_have_no_ambiguous_decision(tc):
    """CPU: the comparator's conditions hold at every step of every stream (train_oracle asserts them), and the resident
    row is read with every gap the issue names"""
    losses, at, ta, rt, tr = train_oracle(tc)
    assert len(losses) == len(INCREMENTS) and all(np.isfinite(losses))
    assert {i - 1 for i in INCREMENTS} == {0, 1, 64, 65}
    assert staged(tc.n, tc.m, tc.o, tc.F) == ("unstaged" not in tc.name)


def dev_state(tc, dev):
    import torch
    at, ta, rt, tr = [T(t, dev) for t in train_start(tc)]
    return [at, ta, torch.zeros(A, dtype=torch.int32, device=dev), rt, tr, torch.zeros(N_ART, dtype=torch.int32, device=dev)]


@gpu
@pytest.mark.parametrize("tc", TRAIN, ids=TIDS)
def test_train_step_vs_dense_oracle(dev, tc, monkeypatch):
    """esr_spotify_train_step (spotify_gather_lazy_kernel, one sort of the 2R virtual rows, kMomentumStepLazy) over a
    playlist stream with sleeping rows, then momentum_flush: every loss, both tables and both traces against the dense
    fp64 run"""
    from esrecsys_amd import ops
    monkeypatch.delenv("ESR_SPOTIFY_CATCHUP", raising=False)
    set_forms(monkeypatch, "default", "default")
    losses, at, ta, rt, tr = train_oracle(tc)
    s = dev_state(tc, dev)
    step = 0
    for (step, album, artist), el in zip(train_stream(tc), losses):
        loss = ops.spotify_train_step(s[0], s[1], s[2], s[3], s[4], s[5], T(album, dev), T(artist, dev), tc.n, tc.m, tc.o,
                                      tc.reg, step, LR, MOM)
        assert abs(float(loss) - el) <= TOL * abs(el), (tc.name, step, float(loss), el)
    assert int((s[2] == step).sum()) <= 2 * (tc.n + tc.m + tc.o) and int((s[2] > step).sum()) == 0
    ops.momentum_flush(s[0], s[1], s[2], step, LR, MOM)
    ops.momentum_flush(s[3], s[4], s[5], step, LR, MOM)
    assert int((s[2] != step).sum()) == 0 and int((s[5] != step).sum()) == 0
    for got, exp, key in ((s[0], at, "album table"), (s[1], ta, "album trace"), (s[3], rt, "artist table"),
                          (s[4], tr, "artist trace")):
        assert rel_err(N(got), exp) <= TOL, (tc.name, key)


@gpu
@pytest.mark.parametrize("tc", TRAIN, ids=TIDS)
def test_inline_catch_up_equals_the_catch_up_launch_over_the_matrix(dev, tc, monkeypatch):
    """test_inline_catch_up_equals_the_catch_up_launch's claim beyond F = 32, n = 5: ESR_SPOTIFY_CATCHUP=launch and the
    default leave bit-identical losses, tables, traces and step marks"""
    import torch
    from esrecsys_amd import ops
    set_forms(monkeypatch, "default", "default")
    a, b = dev_state(tc, dev), dev_state(tc, dev)
    for step, album, artist in train_stream(tc):
        al, ar = T(album, dev), T(artist, dev)
        monkeypatch.setenv("ESR_SPOTIFY_CATCHUP", "launch")
        lb = ops.spotify_train_step(b[0], b[1], b[2], b[3], b[4], b[5], al, ar, tc.n, tc.m, tc.o, tc.reg, step, LR, MOM)
        monkeypatch.setenv("ESR_SPOTIFY_CATCHUP", "inline")
        la = ops.spotify_train_step(a[0], a[1], a[2], a[3], a[4], a[5], al, ar, tc.n, tc.m, tc.o, tc.reg, step, LR, MOM)
        assert float(la) == float(lb), (tc.name, step)
    for x, y in zip(a, b):
        assert torch.equal(x, y), tc.name


# ---------------------------------------------------------------------------------------------- argument checks
@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


EINVAL, EWORKSPACE = -1, -3
P = 256   # a stand-in device address (non-null, aligned): never dereferenced, every call below returns before a launch


def abi_fwd_bwd(lib, n=5, m=17, o=64, F=32, ws=P, ws_bytes=0, rows=A, n_art=N_ART):
    return lib.esr_spotify_fwd_bwd(P, rows, P, n_art, F, P, P, n, m, o, 1.0, P, P, P, P, ws, ws_bytes, None)


def abi_forward(lib, n=5, m=17, o=64, F=32, ws=P, ws_bytes=0, rows=A, n_art=N_ART):
    return lib.esr_spotify_forward(P, rows, P, n_art, F, P, P, n, m, o, P, P, P, P, P, P, ws, ws_bytes, None)


def abi_train_step(lib, n=5, m=17, o=64, F=32, ws=P, ws_bytes=0, rows=A, n_art=N_ART):
    return lib.esr_spotify_train_step(P, P, P, rows, P, P, P, n_art, F, P, P, n, m, o, 1.0, 1, 0.05, 0.9, P, ws, ws_bytes, None)


@pytest.mark.parametrize("call,who,sizer", [(abi_fwd_bwd, b"esr_spotify_fwd_bwd", "esr_spotify_workspace_bytes"),
                                            (abi_forward, b"esr_spotify_forward", "esr_spotify_workspace_bytes"),
                                            (abi_train_step, b"esr_spotify_train_step", "esr_spotify_train_step_workspace_bytes")])
def test_spotify_arguments_are_rejected_without_a_device(lib, call, who, sizer):
    """CPU: sp_check and the workspace check answer before anything is launched (there is no device here to launch on,
    and the pointers are stand-ins): the message names the entry point and the limit; the caps themselves are accepted."""
    def einval(limit, **kw):
        assert call(lib, **kw) == EINVAL, kw
        msg = lib.esr_last_error()
        assert msg.startswith(who + b": bad sizes") and limit in msg, (kw, msg)
        for k, v in kw.items():
            assert (b"%s=%d" % (k.encode(), v)) in msg or k in ("rows", "n_art"), (kw, msg)

    einval(b"n <= 32", n=33)
    einval(b"2F <= 256", F=129)
    einval(b"1 <= n", n=0)
    einval(b"m >= 1", m=0)
    einval(b"o >= 1", o=0)
    einval(b"1 <= F", F=0)
    einval(b"1 <= n", n=-1)
    einval(b"rows >= 1", rows=0)
    einval(b"rows >= 1", n_art=0)
    # the caps are sizes like any other: they get as far as the workspace check
    for kw in ({"n": 32}, {"F": 128}, {"n": 32, "F": 128}, {"n": 1, "m": 1, "o": 1, "F": 1}):
        assert call(lib, **kw) == EWORKSPACE, kw
    # a workspace one byte short, or misaligned: the workspace error with the required size, no launch
    n, m, o, F = 5, 17, 64, 32
    need = getattr(lib, sizer)(n, m, o, F)
    assert need > (n + m + o) * 2 * F * 4
    assert call(lib, ws_bytes=need - 1) == EWORKSPACE
    msg = lib.esr_last_error()
    assert msg.startswith(who + b": workspace") and (b"%d bytes < %d required" % (need - 1, need)) in msg, msg
    assert call(lib, ws=P + 8, ws_bytes=need) == EWORKSPACE
    msg = lib.esr_last_error()
    assert msg.startswith(who + b": workspace") and b"misaligned" in msg and (b"%d required" % need) in msg, msg
    assert call(lib, ws=None, ws_bytes=need) == EINVAL and b"null pointer" in lib.esr_last_error()


@pytest.mark.parametrize("short", [1, -1])
def test_ops_refuse_id_tensors_of_the_wrong_length(short, monkeypatch):
    """CPU: ops.spotify_forward / _fwd_bwd / _train_step raise ValueError when album_ids or artist_ids do not hold exactly
    n + m + o entries -- before the library is even loaded (a short tensor was read past its end on the device)."""
    import torch
    from esrecsys_amd import _lib, ops

    def no_load(*a, **k):
        raise AssertionError("the library was loaded before the id count was checked")
    monkeypatch.setattr(_lib, "load", no_load)
    n, m, o, F = 5, 17, 64, 8
    R = n + m + o
    tab, vec = torch.zeros((16, F)), torch.zeros(16, dtype=torch.int32)
    good, bad = torch.zeros(R, dtype=torch.int32), torch.zeros(R - short, dtype=torch.int32)
    for al, ar, name in ((bad, good, "album_ids"), (good, bad, "artist_ids")):
        msg = r"%s holds %d entries, n \+ m \+ o = 5 \+ 17 \+ 64 = 86" % (name, R - short)
        with pytest.raises(ValueError, match="spotify_forward: " + msg):
            ops.spotify_forward(tab, tab, al, ar, n, m, o)
        with pytest.raises(ValueError, match="spotify_fwd_bwd: " + msg):
            ops.spotify_fwd_bwd(tab, tab, al, ar, n, m, o, 1.0)
        with pytest.raises(ValueError, match="spotify_train_step: " + msg):
            ops.spotify_train_step(tab, tab, vec, tab, tab, vec, al, ar, n, m, o, 1.0, 1, 0.05, 0.9)


@gpu
def test_ops_raise_on_bad_sizes_and_stay_usable(dev):
    """n = 33, F = 129 and empty groups raise EsrLibraryError naming the entry point and the limit; short id tensors
    raise ValueError; the next good call on the same library is correct (the golden case)."""
    import torch
    from esrecsys_amd import _lib, ops
    from test_spotify_oracle import CASES as GOLDEN, batch_of as golden_batch, tables_of

    def tabs(F):
        return torch.zeros((100, F), device=dev), torch.zeros((10, F), device=dev)

    def ids(R):
        return torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)

    def state(F):
        a, r = tabs(F)
        return (a, torch.zeros_like(a), torch.zeros(100, dtype=torch.int32, device=dev), r, torch.zeros_like(r),
                torch.zeros(10, dtype=torch.int32, device=dev))

    for n, m, o, F, limit in ((33, 2, 2, 8, "n <= 32"), (2, 2, 2, 129, "2F <= 256"), (0, 2, 2, 8, "1 <= n"),
                              (2, 0, 2, 8, "m >= 1"), (2, 2, 0, 8, "o >= 1")):
        R = n + m + o
        with pytest.raises(_lib.EsrLibraryError, match=r"esr_spotify_fwd_bwd: bad sizes n=%d m=%d o=%d F=%d .*%s" % (n, m, o, F, limit)):
            ops.spotify_fwd_bwd(*tabs(F), *ids(R), n, m, o, 1.0)
        with pytest.raises(_lib.EsrLibraryError, match=r"esr_spotify_forward: bad sizes n=%d m=%d o=%d F=%d .*%s" % (n, m, o, F, limit)):
            ops.spotify_forward(*tabs(F), *ids(R), n, m, o)
        with pytest.raises(_lib.EsrLibraryError, match=r"esr_spotify_train_step: bad sizes n=%d m=%d o=%d F=%d .*%s" % (n, m, o, F, limit)):
            ops.spotify_train_step(*state(F), *ids(R), n, m, o, 1.0, 1, 0.05, 0.9)
    with pytest.raises(ValueError, match="album_ids holds 5 entries"):
        ops.spotify_fwd_bwd(*tabs(8), *ids(5), 2, 2, 2, 1.0)
    g = load_golden(GOLDEN[0])
    at, rt = tables_of(g, np.float32)
    x = golden_batch(g)
    album = np.concatenate([x["album_context"], x["next_album"], x["neg_album"]]).astype(np.int32)
    artist = np.concatenate([x["artist_context"], x["next_artist"], x["neg_artist"]]).astype(np.int32)
    n, m, o = len(x["album_context"]), len(x["next_album"]), len(x["neg_album"])
    loss, rows, ga, gr = ops.spotify_fwd_bwd(T(at, dev), T(rt, dev), T(album, dev), T(artist, dev), n, m, o, float(g["reg"]))
    assert np.array_equal(N(rows), g["hashed_album"]) and abs(float(loss) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    assert rel_err(N(ga), g["g_album_rows"]) <= TOL and rel_err(N(gr), g["g_artist_rows"]) <= TOL

"""CPU: the NumPy restatement of the Spotify negative sampler (tests/_spotify_sampler_ref.py) against the Random123 known
answers of Philox4x32-10 and the sampler's contract, and esr_philox.h -- the text the kernels compile -- against that
restatement through a stand-alone host program (tests/host/spotify_philox_host.cpp; no HIP, not loaded into Python)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from _spotify_sampler_ref import list_starts, negative_indices, philox4x32_10

# Random123's kat_vectors for philox4x32-10: (counter, key, output)
KAT = [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
REFERENCE_T = 2_262_292


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert _hex(philox4x32_10(counter, key)) == want


def test_philox_is_vectorised_over_counters():
    out = philox4x32_10([[i, 0, 0, 0] for i in range(5)], [0, 0])
    assert out.shape == (5, 4) and out.dtype == np.uint32 and _hex(out[0]) == KAT[0][2]
    assert len({_hex(r) for r in out}) == 5


@pytest.mark.parametrize("T", [2, 3, 13, REFERENCE_T])
def test_every_index_is_below_the_last_track(T):
    for seed, step in ((0, 1), (1701, 1000), (2 ** 64 - 1, 2 ** 31 - 1)):
        idx = negative_indices(seed, step, 4099, T)
        assert idx.dtype == np.int64 and idx.shape == (4099,)
        assert idx.min() >= 0 and idx.max() < T - 1
    if T == 2:
        assert not negative_indices(5, 9, 257, T).any()
    if T == 3:
        assert set(negative_indices(5, 9, 257, T)) == {0, 1}
    if T == REFERENCE_T:   # the map uses the whole range: among 4099 draws the largest is within 1 % of the end
        assert negative_indices(0, 1, 4099, T).max() > 0.99 * (T - 1)


def test_a_prefix_of_a_longer_draw_is_the_shorter_draw():
    """negative i depends on (seed, step, i) alone: 1, 5 (a partial Philox block past one) and 64 agree where they overlap"""
    full = negative_indices(42, 7, 64, 13)
    for o in (1, 5, 63):
        assert np.array_equal(negative_indices(42, 7, o, 13), full[:o])


def test_steps_and_seeds_give_different_lists():
    T, o = REFERENCE_T, 64
    lists = [tuple(negative_indices(seed, step, o, T)) for seed in (0, 1, 1701) for step in (1, 2, 1000, 1001)]
    assert len(set(lists)) == len(lists)
    assert tuple(negative_indices(0, 1, o, T)) == lists[0]          # and the same (seed, step) the same list


def test_a_64_bit_seed_uses_both_key_words():
    T, o, lo = REFERENCE_T, 64, 0x9E3779B9
    a = negative_indices(lo, 3, o, T)
    b = negative_indices(lo | (1 << 32), 3, o, T)                   # same low word, another high word
    c = negative_indices(lo | (1 << 63), 3, o, T)
    d = negative_indices((lo + 1) & 0xFFFFFFFF, 3, o, T)            # another low word
    assert len({tuple(v) for v in (a, b, c, d)}) == 4
    # the key is (seed & 0xffffffff, seed >> 32)
    words = philox4x32_10([0, 3, 0, 0], [lo, 1])
    assert int(b[1]) == (int(words[1]) * (T - 1)) >> 32
    assert np.array_equal(negative_indices(lo + (1 << 64), 3, o, T), a)   # seeds are taken mod 2^64


def test_multiply_high_bias_is_what_the_docstring_says():
    """(word * (T - 1)) >> 32 gives every index floor or ceil of 2^32 / (T - 1) words: relative bias <= (T - 1) / 2^32."""
    from esrecsys_amd.spotify.train_spotify import NegativeSampler
    assert (REFERENCE_T - 1) / 2 ** 32 <= 5.3e-4
    assert "5.3e-4" in NegativeSampler.__doc__ and "2^32" in NegativeSampler.__doc__
    t1 = 12                                                         # exhaustive over a 16-bit analogue: words 0 .. 2^16 - 1
    counts = np.bincount((np.arange(1 << 16, dtype=np.uint64) * np.uint64(t1)) >> np.uint64(16), minlength=t1)
    assert counts.max() - counts.min() <= 1 and counts.sum() == 1 << 16


def test_list_starts_are_aligned_and_disjoint():
    rng = np.random.default_rng(0)
    for n, o in ((1, 1), (5, 64), (5, 5), (32, 63)):
        lens = rng.choice([1, 3, 40], 9)
        off = np.concatenate([[0], np.cumsum(lens)])
        s = list_starts(n, off, o)
        R = n + lens + o
        assert (s % 64 == 0).all() and s[0] == 0
        assert (s[1:] >= s[:-1] + 2 * R[:-1]).all()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("philox") / "philox_host")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tests", "host", "spotify_philox_host.cpp"), "-o", exe],
                   check=True)
    return exe


def test_the_header_computes_what_the_restatement_computes(host_program):
    """esr_philox.h, compiled for the host: the three known answers, sampler indices at every corpus size above, the
    offsets validation and the list layout."""
    quads = [(0, 1, 64, 13), (0x123456789ABCDEF, 1000, 9, 13), (2 ** 64 - 1, 2 ** 31 - 1, 5, 2), (7, 3, 70, 3),
             (1701, 123456, 67, REFERENCE_T), (1 << 32, 1, 8, 2 ** 31)]
    args = [str(v) for q in quads for v in q]
    out = subprocess.run([host_program] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert [l[4:] for l in out if l.startswith("kat ")] == [k[2] for k in KAT]
    got = [np.array(l.split()[1:], dtype=np.int64) for l in out if l.startswith("idx")]
    assert len(got) == len(quads)
    for g, (seed, step, count, T) in zip(got, quads):
        assert np.array_equal(g, negative_indices(seed, step, count, T)), (seed, step, count, T)
    checks = [tuple(int(v) for v in l.split()[1:]) for l in out if l.startswith("offsets")]
    assert checks == [(0, 3), (0, 40), (1, -1), (3, -1), (3, -1), (2, -1), (0, 2 ** 63 - 1), (3, -1), (1, -1)]
    starts = [l.split() for l in out if l.startswith("starts")][0]
    want = list_starts(5, [0, 1, 4, 44], 64)
    assert [int(v) for v in starts[1:4]] == list(want)
    assert int(starts[-1]) >= want[-1] + 2 * (5 + 40 + 64)

"""CPU: the Spotify group-step entry points (esr_spotify_sample_negatives, esr_spotify_train_steps and its workspace
query) are declared, bound and exported, and reject bad arguments with their codes before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from _spotify_sampler_ref import list_starts

EINVAL, EWORKSPACE = -1, -3
A = 0x10000   # a 256-byte aligned address that is never dereferenced: every call below fails validation first
NEW = ["esr_spotify_sample_negatives", "esr_spotify_train_steps", "esr_spotify_train_steps_workspace_bytes"]


@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from esrecsys_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "esr_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(esr_[a-z0-9_]+)\s*\(", text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert "`%s`" % name in doc, name
    # the bound argument counts are the header's
    for name in NEW:
        proto = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name


def _offsets(lens):
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return off


def _steps(lib, album=A, rows=7, artist=A, n_art=11, F=4, n=5, o=5, K=None, ctx=A, nxt=A, off=(1, 3, 40), off_ptr="host",
           off_dev=A, corpus=A, T=13, seed=1, first_step=1, losses=A, neg_index=None, ws=A, ws_bytes=None, trace=A, last=A):
    off = np.ascontiguousarray(off if isinstance(off, np.ndarray) else _offsets(off))
    K = off.size - 1 if K is None else K
    if ws_bytes is None:
        lens = np.diff(off)
        ws_bytes = lib.esr_spotify_train_steps_workspace_bytes(max(n, 1), max(int(lens.max()), 1), max(o, 1), max(F, 1),
                                                               max(K, 1), max(int(off[-1]), K))
    host = off.ctypes.data if off_ptr == "host" else off_ptr
    return lib.esr_spotify_train_steps(album, trace, last, rows, artist, trace, last, n_art, F, n, o, K, ctx, ctx, nxt, nxt,
                                       host, off_dev, corpus, corpus, T, seed, first_step, 10.0, 1e-3, 0.98, losses,
                                       neg_index, ws, ws_bytes, None)


def test_train_steps_rejects_bad_arguments_without_a_device(lib):
    def einval(msg, **kw):
        assert _steps(lib, **kw) == EINVAL, kw
        assert msg in lib.esr_last_error(), (kw, lib.esr_last_error())

    for kw in ({"n": 0}, {"n": 33}, {"o": 0}, {"F": 0}, {"F": 129}, {"rows": 0}, {"n_art": 0}):
        einval(b"bad sizes", **kw)
    einval(b"K=0", K=0)
    einval(b"K=-1", K=-1)
    einval(b"first_step=0", first_step=0)
    einval(b"first_step=-5", first_step=-5)
    einval(b"last step", first_step=2 ** 31 - 2)                    # first_step + K - 1 = 2^31: no int
    einval(b"T=1", T=1)
    einval(b"T=0", T=0)
    einval(b"T=2147483649", T=2 ** 31 + 1)                          # T - 1 > 2^31 - 1
    for name in ("album", "artist", "trace", "last", "ctx", "nxt", "off_dev", "corpus", "losses", "ws"):
        einval(b"null pointer", **{name: None})
    einval(b"null pointer", off_ptr=None)
    # offsets: from 0, strictly increasing (an empty next list is m = 0)
    einval(b"next_offsets[0]", off=np.array([1, 2, 3], dtype=np.int64))
    einval(b"next_offsets[2] = 1", off=np.array([0, 1, 1, 4], dtype=np.int64))      # an empty list
    einval(b"next_offsets[3] = 2", off=np.array([0, 1, 3, 2], dtype=np.int64))      # non-monotone
    einval(b"next_offsets[1] = -4", off=np.array([0, -4], dtype=np.int64))
    # more than 2^24 ids in one group: K (n + o) + total_next
    big = np.array([0, 2 ** 24 - 10 + 1], dtype=np.int64)
    einval(b"exceed 2^24", off=big, ws_bytes=1 << 40)
    assert _steps(lib, off=np.array([0, 2 ** 24 - 10], dtype=np.int64), ws_bytes=0) == EWORKSPACE   # exactly 2^24 passes
    einval(b"tables too large", rows=1 << 30)


def test_train_steps_workspace_is_checked_before_any_launch(lib):
    n, o, F, lens = 5, 64, 32, (1, 3, 40)
    off = _offsets(lens)
    need = lib.esr_spotify_train_steps_workspace_bytes(n, 40, o, F, 3, int(off[-1]))
    assert _steps(lib, n=n, o=o, F=F, off=lens, ws_bytes=need - 1) == EWORKSPACE
    assert b"workspace" in lib.esr_last_error()
    assert _steps(lib, n=n, o=o, F=F, off=lens, ws=A + 4) == EWORKSPACE                 # misaligned
    assert _steps(lib, n=n, o=o, F=F, off=lens, ws_bytes=0) == EWORKSPACE
    # the limits themselves pass validation and stop at the workspace
    assert _steps(lib, n=32, F=128, o=1, off=(1,), T=2, ws_bytes=0) == EWORKSPACE
    assert _steps(lib, T=2 ** 31, first_step=2 ** 31 - 3, ws_bytes=0) == EWORKSPACE     # last step = 2^31 - 1
    # the workspace = the id lists (the documented layout) + one step's workspace at the longest list
    starts = list_starts(n, off, o)
    lists_ints = starts[-1] + 2 * (n + lens[-1] + o)
    step = lib.esr_spotify_train_step_workspace_bytes(n, 40, o, F)
    assert step + 4 * lists_ints <= need <= step + 4 * lists_ints + 256 * (len(lens) + 2)
    for m in (1, 3, 40):   # every shorter list fits the region sized for the longest
        assert lib.esr_spotify_train_step_workspace_bytes(n, m, o, F) <= step
    assert lib.esr_spotify_train_steps_workspace_bytes(0, 1, 1, 1, 1, 1) == 256
    assert lib.esr_spotify_train_steps_workspace_bytes(5, 250, 64, 32, 64, 64 * 250) < 1 << 22    # a group is small


def _sample(lib, albums=A, artists=A, T=13, seed=1, step=1, o=5, idx=A, al=A, ar=A):
    return lib.esr_spotify_sample_negatives(albums, artists, T, seed, step, o, idx, al, ar, None)


def test_sample_negatives_rejects_bad_arguments_without_a_device(lib):
    for kw, msg in (({"T": 1}, b"T=1"), ({"T": 0}, b"T=0"), ({"T": 2 ** 31 + 1}, b"T=2147483649"), ({"o": 0}, b"o=0"),
                    ({"o": 2 ** 24 + 1}, b"bad sizes"), ({"step": 0}, b"step=0"), ({"step": -1}, b"step=-1"),
                    ({"albums": None}, b"null pointer"), ({"artists": None}, b"null pointer"),
                    ({"idx": None, "al": None, "ar": None}, b"null pointer")):
        assert _sample(lib, **kw) == EINVAL, kw
        assert msg in lib.esr_last_error(), (kw, lib.esr_last_error())
        assert b"esr_spotify_sample_negatives" in lib.esr_last_error()


def test_python_layer_checks_before_the_library():
    from esrecsys_amd import spotify
    from esrecsys_amd.spotify.train_spotify import NegativeSampler, train_steps
    assert spotify.NegativeSampler is NegativeSampler and spotify.train_steps is train_steps
    trk = np.arange(6)
    with pytest.raises(ValueError, match="differ in length"):
        NegativeSampler(trk, trk[:5], trk, 4, 0, 10, "cpu")
    with pytest.raises(ValueError, match="T >= 2"):
        NegativeSampler(trk[:1], trk[:1], trk[:1], 4, 0, 10, "cpu")
    with pytest.raises(ValueError, match="num_negatives"):
        NegativeSampler(trk, trk, trk, 0, 0, 10, "cpu")
    with pytest.raises(IndexError, match=r"\[0, 5\)"):
        NegativeSampler(trk, trk, trk, 4, 0, 5, "cpu")               # artist 5 of a 5-artist table
    x = {"album_context": np.arange(5), "artist_context": np.arange(5), "next_album": np.arange(3), "next_artist": np.arange(3)}
    y = dict(x, album_context=np.arange(4), artist_context=np.arange(4))
    with pytest.raises(ValueError, match="one context length"):
        train_steps(None, iter([x, y]), 2, 10.0, None)
    with pytest.raises(ValueError, match=">= 1"):
        train_steps(None, iter([x]), 0, 10.0, None)
    assert isinstance(ctypes.c_uint64(2 ** 64 - 1).value, int)

"""CPU: the batched Spotify eval entry point (esr_spotify_topk_batch) rejects bad arguments before it touches a device,
its workspace holds no [P, T] score matrix, and the Python layer refuses batches it cannot score in one call."""
import os

import numpy as np
import pytest

EINVAL, EWORKSPACE = -1, -3
A = 0x10000   # a 16-byte aligned address that is never dereferenced: every call below fails validation first


@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


def _call(lib, album=A, rows=1000, artist=A, n_art=500, F=32, ca=A, cr=A, P=4, n=5, aa=A, ar=A, T=10_000, k=100,
          out_s=A, out_i=A, ws=A, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.esr_spotify_topk_batch_workspace_bytes(max(P, 1), max(n, 1), max(T, 1), max(F, 1), max(k, 1))
    return lib.esr_spotify_topk_batch(album, rows, artist, n_art, F, ca, cr, P, n, aa, ar, T, k, out_s, out_i, ws,
                                      ws_bytes, None)


def test_bad_arguments_are_rejected_without_a_device(lib):
    assert _call(lib, n=0) == EINVAL
    assert b"bad sizes" in lib.esr_last_error()
    assert _call(lib, n=33) == EINVAL
    assert _call(lib, F=129) == EINVAL                       # 2F > 256
    assert _call(lib, F=0) == EINVAL
    assert _call(lib, k=0) == EINVAL
    assert b"k=0" in lib.esr_last_error()
    assert _call(lib, k=101, T=100) == EINVAL                # k > T
    assert _call(lib, k=1025, T=100_000) == EINVAL           # k > 1024
    assert _call(lib, P=0) == EINVAL
    assert _call(lib, T=0) == EINVAL
    assert _call(lib, rows=0) == EINVAL
    assert _call(lib, n_art=0) == EINVAL
    for name in ("album", "artist", "ca", "cr", "aa", "ar", "out_s", "out_i", "ws"):
        assert _call(lib, **{name: None}) == EINVAL, name
        assert b"null pointer" in lib.esr_last_error()
    # a workspace smaller than the query: the project's workspace code, before any launch
    full = lib.esr_spotify_topk_batch_workspace_bytes(4, 5, 10_000, 32, 100)
    assert _call(lib, ws_bytes=full - 1) == EWORKSPACE
    assert b"workspace" in lib.esr_last_error()
    assert _call(lib, ws=A + 4) == EWORKSPACE                # misaligned


def test_the_limits_themselves_are_accepted_as_far_as_the_workspace(lib):
    """n = 32, 2F = 256, k = T = 1024 and P = 1 pass validation (and stop at the workspace check with no workspace)."""
    assert _call(lib, n=32, F=128, k=1024, T=1024, P=1, ws_bytes=0) == EWORKSPACE
    assert _call(lib, n=1, F=1, k=1, T=1, ws_bytes=0) == EWORKSPACE


def test_workspace_at_the_reference_shape_is_not_a_score_matrix(lib, monkeypatch):
    monkeypatch.delenv("ESR_SPOTIFY_EVAL_CHUNK", raising=False)
    P, n, T, F, k = 1000, 5, 2_262_292, 32, 500
    nb = lib.esr_spotify_topk_batch_workspace_bytes(P, n, T, F, k)
    assert 0 < nb <= 2 << 30
    assert nb < P * T * 4 // 4
    # a one-chunk corpus needs no lists: the dense scores of that chunk and the context rows only
    assert lib.esr_spotify_topk_batch_workspace_bytes(3, 5, 600, 32, 500) < 64 << 10
    # the chunk hook shrinks the lists
    monkeypatch.setenv("ESR_SPOTIFY_EVAL_CHUNK", "4096")
    assert lib.esr_spotify_topk_batch_workspace_bytes(P, n, T, F, k) < nb


def _y(n, seed):
    rng = np.random.default_rng(seed)
    return {"album_context": rng.integers(0, 1000, n), "artist_context": rng.integers(0, 100, n),
            "next_track": rng.integers(0, 10, 3), "next_artist": rng.integers(0, 10, 3)}


def test_python_layer_refuses_mixed_context_lengths_and_an_empty_batch():
    from esrecsys_amd.spotify.train_spotify import all_track_top_k_batch, eval_batch, eval_steps
    albums, artists = np.arange(50), np.arange(50)
    with pytest.raises(ValueError, match="empty"):
        all_track_top_k_batch(None, [], albums, artists)
    with pytest.raises(ValueError, match="one context length"):
        all_track_top_k_batch(None, [_y(5, 0), _y(4, 1)], albums, artists)
    with pytest.raises(ValueError, match="one context length"):
        eval_batch(None, [_y(5, 0), _y(5, 1), _y(6, 2)], np.arange(50), albums, artists)
    bad = _y(5, 3)
    bad["artist_context"] = bad["artist_context"][:3]        # albums and artists of one playlist disagree
    with pytest.raises(ValueError, match="one context length"):
        all_track_top_k_batch(None, [bad], albums, artists)
    with pytest.raises(ValueError):
        eval_steps(None, iter([]), 0, np.arange(50), albums, artists)

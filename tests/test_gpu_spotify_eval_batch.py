"""GPU: the batched Spotify eval (esr_spotify_eval.hip, esr_spotify_topk_batch) against the per-playlist path it
replaces (all_track_top_k / eval_step: esr_spotify_affinity_all + two top-k merges), bit for bit, across its geometry
(F, n, P, k, T, chunk plan), on ties, at the reference size against the fp64 oracle, and through the eval loop."""
import types

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import spotify as o_sp

pytestmark = pytest.mark.gpu
TOL = 1e-5
F64 = np.float64


def N(t):
    return t.detach().cpu().numpy()


def _state(at, rt):
    return types.SimpleNamespace(params={"params": {"album_embed": {"embedding": at}, "artist_embed": {"embedding": rt}}})


def _corpus(rng, T, A, n_art, album_range=700_000):
    return rng.integers(0, album_range, T).astype(np.int32), rng.integers(0, n_art, T).astype(np.int32)


def _playlists(rng, P, n, all_albums, all_artists, n_next=(1, 12)):
    ys = []
    T = len(all_albums)
    for _ in range(P):
        pick = rng.integers(0, T, n)
        nx = rng.integers(0, T, int(rng.integers(n_next[0], n_next[1] + 1)))
        ys.append({"album_context": all_albums[pick], "artist_context": all_artists[pick],
                   "next_track": nx.astype(np.int32), "next_artist": all_artists[nx]})
    return ys


def _assert_equal_to_per_playlist(state, ys, d_alb, d_art, k):
    from esrecsys_amd.spotify.train_spotify import all_track_top_k, all_track_top_k_batch
    s, i = all_track_top_k_batch(state, ys, d_alb, d_art, k=k)
    assert s.shape == i.shape == (len(ys), min(k, d_alb.numel()))
    for p, y in enumerate(ys):
        es, ei = all_track_top_k(state, y, d_alb, d_art, k=k)
        assert torch.equal(s[p], es) and torch.equal(i[p], ei), p


# (F, n, P, k, T, tracks per filtered chunk or None)
GEOMETRY = [
    (32, 5, 64, 500, 200_003, None),
    (32, 5, 300, 10, 200_003, "5000"),
    (2, 1, 3, 1, 1, None),                 # T = k = 1, the scalar order
    (5, 32, 3, 10, 11, None),              # T = k + 1
    (16, 5, 1, 1024, 1024, None),          # T = k = 1024
    (64, 5, 64, 1024, 1025, None),
    (128, 32, 3, 500, 200_003, "3000"),    # 2F = 256, n = 32, many chunks
    (5, 5, 64, 500, 200_003, "20000"),     # the scalar order over chunks
    (32, 32, 300, 1024, 200_003, None),
    (2, 1, 1, 500, 200_003, None),
    (32, 5, 3, 500, 30_000, "64"),         # chunks shorter than the compaction mark
]


@pytest.mark.parametrize("F,n,P,k,T,chunk", GEOMETRY)
def test_batch_equals_per_playlist_across_the_geometry(dev, monkeypatch, F, n, P, k, T, chunk):
    if chunk is None:
        monkeypatch.delenv("ESR_SPOTIFY_EVAL_CHUNK", raising=False)
    else:
        monkeypatch.setenv("ESR_SPOTIFY_EVAL_CHUNK", chunk)
    rng = np.random.default_rng(F * 1000 + n * 10 + P + k)
    A, n_art = 20_000, 3000
    g = torch.Generator(device=dev).manual_seed(F + n)
    at = torch.randn((A, F), generator=g, device=dev) * 0.3
    rt = torch.randn((n_art, F), generator=g, device=dev) * 0.3
    all_albums, all_artists = _corpus(rng, T, A, n_art)
    ys = _playlists(rng, P, n, all_albums, all_artists)
    _assert_equal_to_per_playlist(_state(at, rt), ys, torch.from_numpy(all_albums).to(dev),
                                  torch.from_numpy(all_artists).to(dev), k)


@pytest.mark.parametrize("F,chunk", [(32, "3000"), (5, "3000"), (32, None)])
def test_ties_and_zero_rows_equal_per_playlist(dev, monkeypatch, F, chunk):
    """A corpus of a few dozen (album, artist) pairs: thousands of tracks tie exactly, so every chunk appends to the
    lists and they are compacted.  Albums that collide mod A differ in raw id (only the boost separates them); context
    lists repeat a track; some rows are all zero."""
    if chunk is None:
        monkeypatch.delenv("ESR_SPOTIFY_EVAL_CHUNK", raising=False)
    else:
        monkeypatch.setenv("ESR_SPOTIFY_EVAL_CHUNK", chunk)
    rng = np.random.default_rng(9)
    A, n_art, T = 1000, 50, 60_000
    g = torch.Generator(device=dev).manual_seed(5)
    at = torch.randn((A, F), generator=g, device=dev)
    rt = torch.randn((n_art, F), generator=g, device=dev)
    at[:5] = 0.0
    rt[:5] = 0.0
    at[7] = -0.0
    base = rng.integers(0, 10, 40)
    pair_album = (base + A * rng.integers(0, 3, 40)).astype(np.int32)   # 10 table rows, up to 3 raw ids each
    pair_artist = rng.integers(0, 12, 40).astype(np.int32)
    which = rng.integers(0, 40, T)
    all_albums, all_artists = pair_album[which], pair_artist[which]
    ys = _playlists(rng, 40, 5, all_albums, all_artists)
    for p in range(0, 40, 4):
        ys[p]["album_context"] = np.repeat(ys[p]["album_context"][:1], 5)
        ys[p]["artist_context"] = np.repeat(ys[p]["artist_context"][:1], 5)
    for p in range(1, 40, 5):                        # a context of zero rows: every dot product is +0
        ys[p]["album_context"] = np.array([0, 1, A, 2, 3], np.int32)
        ys[p]["artist_context"] = np.array([0, 1, 2, 3, 4], np.int32)
    _assert_equal_to_per_playlist(_state(at, rt), ys, torch.from_numpy(all_albums).to(dev),
                                  torch.from_numpy(all_artists).to(dev), 500)


def test_reference_size_against_the_fp64_oracle(dev, monkeypatch):
    from esrecsys_amd.spotify.train_spotify import all_track_top_k, all_track_top_k_batch
    monkeypatch.delenv("ESR_SPOTIFY_EVAL_CHUNK", raising=False)
    rng = np.random.default_rng(2026)
    T, A, n_art, F, P = 2_262_292, 100_000, 295_861, 32, 64
    g = torch.Generator(device=dev).manual_seed(11)
    at = torch.randn((A, F), generator=g, device=dev) * 0.2
    rt = torch.randn((n_art, F), generator=g, device=dev) * 0.2
    all_albums, all_artists = _corpus(rng, T, A, n_art, 734_684)
    d_alb, d_art = torch.from_numpy(all_albums).to(dev), torch.from_numpy(all_artists).to(dev)
    ys = _playlists(rng, P, 5, all_albums, all_artists)
    state = _state(at, rt)
    s, i = all_track_top_k_batch(state, ys, d_alb, d_art)
    for p in range(0, P, 8):
        es, ei = all_track_top_k(state, ys[p], d_alb, d_art)
        assert torch.equal(s[p], es) and torch.equal(i[p], ei), p
    at64, rt64 = N(at).astype(F64), N(rt).astype(F64)
    for p in (0, 21, 42, 63):
        aff = o_sp.all_track_affinity(at64, rt64, ys[p], all_albums, all_artists)
        _, eidx = o_sp.eval_step(at64, rt64, ys[p], np.arange(T), all_albums, all_artists, k=500)
        got = N(i[p]).astype(np.int64)
        assert rel_err(N(s[p]), aff[eidx]) <= TOL, p
        assert np.mean(got == eidx) > 0.99 and rel_err(aff[got], aff[eidx]) <= TOL, p


def _world(dev, T=200_003, n_art=4000, seed=4):
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.spotify.models import SpotifyModel
    rng = np.random.default_rng(seed)
    model = SpotifyModel(feature_size=32, device=dev, num_artists=n_art)
    all_tracks = (np.arange(T, dtype=np.int64) * 7 + 3).astype(np.int32)      # track ids are not positions
    all_albums, all_artists = _corpus(rng, T, 100_000, n_art)
    return model, rng, all_tracks, all_albums, all_artists, TrainState, optim


def _eval_playlists(rng, state, P, all_tracks, all_albums, all_artists):
    """ragged next lists of 1-250 tracks, some repeated, some among the 500 best, most not"""
    from esrecsys_amd.spotify.train_spotify import all_track_top_k
    T = len(all_tracks)
    ys = []
    for p in range(P):
        pick = rng.integers(0, T, 5)
        y = {"album_context": all_albums[pick], "artist_context": all_artists[pick]}
        _, top = all_track_top_k(state, y, all_albums, all_artists)
        top = N(top).astype(np.int64)
        m = int(rng.integers(1, 251)) if p % 3 else int(rng.integers(1, 4))
        nx = np.concatenate([rng.choice(top, int(rng.integers(0, min(m, 40) + 1))), rng.integers(0, T, m)])[:m]
        if m > 2:
            nx[-1] = nx[0]                                                   # a repeated next track
        y["next_track"] = all_tracks[nx]
        y["next_artist"] = all_artists[nx]
        ys.append(y)
    return ys


def test_eval_batch_equals_eval_step(dev):
    from esrecsys_amd.spotify.train_spotify import eval_batch, eval_step
    model, rng, all_tracks, all_albums, all_artists, TrainState, optim = _world(dev)
    state = TrainState.create(apply_fn=model.apply, params=model.init(1701), tx=optim.sgd(1e-3, 0.98))
    ys = _eval_playlists(rng, state, 60, all_tracks, all_albums, all_artists)
    got = eval_batch(state, ys, all_tracks, all_albums, all_artists)
    want = torch.stack([eval_step(state, y, all_tracks, all_albums, all_artists) for y in ys])
    assert got.shape == (60, 2) and got.dtype == torch.float32
    assert torch.equal(got, want)
    assert float(want[:, 0].max()) > 0 and float(want[:, 1].max()) > 0          # recall that is not all zero
    # next lists handed over as device tensors take the same path
    dys = [{key: torch.from_numpy(np.asarray(v)).to(dev) for key, v in y.items()} for y in ys[:10]]
    assert torch.equal(eval_batch(state, dys, all_tracks, all_albums, all_artists), want[:10])


def test_eval_steps_equals_the_reference_loop(dev):
    from esrecsys_amd.spotify.train_spotify import eval_step, eval_steps
    model, rng, all_tracks, all_albums, all_artists, TrainState, optim = _world(dev)
    state = TrainState.create(apply_fn=model.apply, params=model.init(1701), tx=optim.sgd(1e-3, 0.98))
    ys = _eval_playlists(rng, state, 50, all_tracks, all_albums, all_artists)
    for steps, batch in ((37, 16), (50, 256), (1, 4)):
        it = iter(ys)
        got = eval_steps(state, it, steps, all_tracks, all_albums, all_artists, batch=batch)
        assert next(it) is ys[steps] if steps < len(ys) else next(it, None) is None
        sum_metrics = torch.zeros(2, dtype=torch.float32, device=dev)      # train_spotify.py:270-275
        ref_it = iter(ys)
        for _ in range(steps):
            sum_metrics = sum_metrics + eval_step(state, next(ref_it), all_tracks, all_albums, all_artists)
        assert torch.equal(got, sum_metrics / steps), (steps, batch)


def test_lazy_momentum_is_undisturbed_by_the_batched_eval(dev):
    from esrecsys_amd.spotify.train_spotify import eval_batch, eval_step, sample_negative, train_step
    model, rng, all_tracks, all_albums, all_artists, TrainState, optim = _world(dev, seed=8)
    params = model.init(1701)
    clone = lambda tree: {"params": {k: {"embedding": v["embedding"].clone()} for k, v in tree["params"].items()}}  # noqa: E731
    a = TrainState.create(apply_fn=model.apply, params=clone(params), tx=optim.sgd(1e-3, 0.98))
    b = TrainState.create(apply_fn=model.apply, params=clone(params), tx=optim.sgd(1e-3, 0.98))
    T = len(all_tracks)
    xs = []
    for _ in range(40):
        pick = rng.integers(0, T, 5 + 12)
        x = {"track_context": all_tracks[pick[:5]], "album_context": all_albums[pick[:5]],
             "artist_context": all_artists[pick[:5]], "next_track": all_tracks[pick[5:]],
             "next_album": all_albums[pick[5:]], "next_artist": all_artists[pick[5:]]}
        sample_negative(x, rng, 64, all_tracks, all_albums, all_artists)
        xs.append(x)
    ys = [{"album_context": x["album_context"], "artist_context": x["artist_context"], "next_track": x["next_track"],
           "next_artist": x["next_artist"]} for x in xs[:12]]
    for x in xs[:20]:
        a, la = train_step(a, x, 10.0)
        b, lb = train_step(b, x, 10.0)
    ma = eval_batch(a, ys, all_tracks, all_albums, all_artists)
    mb = torch.stack([eval_step(b, y, all_tracks, all_albums, all_artists) for y in ys])
    assert torch.equal(ma, mb)
    for x in xs[20:]:
        a, la = train_step(a, x, 10.0)
        b, lb = train_step(b, x, 10.0)
        assert float(la) == float(lb)
    for key in ("album_embed", "artist_embed"):
        assert torch.equal(a.raw_params["params"][key]["embedding"], b.raw_params["params"][key]["embedding"])
        assert torch.equal(a.opt_state["trace"]["params"][key]["embedding"], b.opt_state["trace"]["params"][key]["embedding"])
        last = ("params", key, "embedding")
        assert torch.equal(a.opt_state["_lazy"]["last"][last], b.opt_state["_lazy"]["last"][last])


def test_the_split_of_a_batch_does_not_matter(dev, monkeypatch):
    from esrecsys_amd.spotify.train_spotify import all_track_top_k_batch
    monkeypatch.delenv("ESR_SPOTIFY_EVAL_CHUNK", raising=False)
    rng = np.random.default_rng(300)
    A, n_art, F, T = 50_000, 3000, 32, 200_003
    g = torch.Generator(device=dev).manual_seed(300)
    at = torch.randn((A, F), generator=g, device=dev) * 0.3
    rt = torch.randn((n_art, F), generator=g, device=dev) * 0.3
    all_albums, all_artists = _corpus(rng, T, A, n_art)
    d_alb, d_art = torch.from_numpy(all_albums).to(dev), torch.from_numpy(all_artists).to(dev)
    ys = _playlists(rng, 300, 5, all_albums, all_artists)
    state = _state(at, rt)
    s, i = all_track_top_k_batch(state, ys, d_alb, d_art)
    parts = [all_track_top_k_batch(state, ys[j:j + 100], d_alb, d_art) for j in (0, 100, 200)]
    assert torch.equal(s, torch.cat([q[0] for q in parts])) and torch.equal(i, torch.cat([q[1] for q in parts]))

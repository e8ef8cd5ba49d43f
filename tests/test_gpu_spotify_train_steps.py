"""GPU: the Spotify group call (train_steps / esr_spotify_train_steps) and the device-side negative sampler.

Tiny world on purpose: 7 album rows (raw album ids up to 59, so `album mod rows` collides), 11 artists, a corpus of T = 13
tracks -- every step shares rows with its neighbours; with one negative and short next lists most rows rest for several
steps and are caught up when they return (rows_rest_and_return checks that on the host).  The sampler is compared with
the NumPy restatement (tests/_spotify_sampler_ref.py) exactly; the group call with the per-playlist loop bit for bit; and
three steps with the fp64 oracle at the per-step oracle test's tolerance (test_gpu_spotify.TOL): the group call adds no
arithmetic of its own, so it gets no margin beyond it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, rel_err
from oracle import spotify as o_sp
from _spotify_sampler_ref import list_starts, negative_indices
from test_gpu_spotify import TOL

pytestmark = pytest.mark.gpu
F64 = np.float64
ROWS, N_ART, T = 7, 11, 13
SEED = 0x5EED0123456789AB            # both key words in use
LR, MOM, REG = 0.05, 0.9, 0.9
LENS = {1: [3], 2: [40, 1], 3: [3, 40, 1], 9: [3, 1, 1, 3, 1, 1, 3, 1, 40]}   # next-list lengths, ragged within a group
PATHS = {"album_embed": ("params", "album_embed", "embedding"), "artist_embed": ("params", "artist_embed", "embedding")}


def corpus():
    rng = np.random.default_rng(13)
    return np.arange(T, dtype=np.int64) + 1000, rng.integers(0, 60, T), rng.integers(0, N_ART, T)


def playlists(n, K, seed=0):
    """K feature dicts (host arrays, no negatives) drawn from the corpus: n context tracks, LENS[K][j] next tracks."""
    tracks, albums, artists = corpus()
    rng = np.random.default_rng(1000 * n + 10 * K + seed)
    out = []
    for m in LENS[K]:
        pick = rng.integers(0, T, n + m)
        out.append({"track_context": tracks[pick[:n]], "album_context": albums[pick[:n]], "artist_context": artists[pick[:n]],
                    "next_track": tracks[pick[n:]], "next_album": albums[pick[n:]], "next_artist": artists[pick[n:]]})
    return out


def with_negatives(x, step, o):
    """x plus the negatives the sampler must draw for `step` (host arrays, from the NumPy restatement)"""
    tracks, albums, artists = corpus()
    idx = negative_indices(SEED, step, o, T)
    return dict(x, neg_track=tracks[idx], neg_album=albums[idx], neg_artist=artists[idx])


def rows_rest_and_return(xs, first_step, o, gap=3):
    """some artist row is read, not read by the next `gap` steps or more, and then read again"""
    seen = {}
    for j, x in enumerate(xs):
        f = with_negatives(x, first_step + j, o)
        for a in set(np.concatenate([f["artist_context"], f["next_artist"], f["neg_artist"]]).tolist()):
            if a in seen and j - seen[a] > gap:
                return True
            seen[a] = j
    return False


def new_state(dev, F, first_step=1, lazy=True):
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.spotify.models import SpotifyModel
    model = SpotifyModel(feature_size=F, device=dev, max_albums=ROWS, num_artists=N_ART)
    state = TrainState.create(apply_fn=model.apply, params=model.init(1701), tx=optim.sgd(LR, MOM, lazy=lazy))
    if lazy:
        state.tx._lazy_state(state.raw_params, state.opt_state)["step"] = first_step - 1   # (a restored run's counter)
    return state


def new_sampler(dev, o):
    from esrecsys_amd.spotify.train_spotify import NegativeSampler
    return NegativeSampler(*corpus(), o, SEED, N_ART, dev)


def tensors_of(state):
    """every tensor a step writes, unflushed: tables, traces, last"""
    raw, tr = state.raw_params["params"], state.opt_state["trace"]["params"]
    out = {}
    for k, path in PATHS.items():
        out[k + ".table"], out[k + ".trace"] = raw[k]["embedding"], tr[k]["embedding"]
        lz = state.opt_state.get("_lazy")
        if lz is not None:
            out[k + ".last"] = lz["last"][path]
    return out


def group_vs_loop(dev, F, n, o, K, first_step, group):
    """train_steps over K playlists against sampler.fill + train_step K times, from identical states: torch.equal on
    both tables, both traces, both `last` arrays, the step counters and all K losses.  Returns the group run's state."""
    from esrecsys_amd.spotify.train_spotify import train_step, train_steps
    xs = playlists(n, K)
    sampler = new_sampler(dev, o)
    a, b = new_state(dev, F, first_step), new_state(dev, F, first_step)
    a, la = train_steps(a, iter([dict(x) for x in xs]), K, REG, sampler, group=group)
    lb = []
    for j, x in enumerate(xs):
        b, l = train_step(b, sampler.fill(dict(x), first_step + j), REG)
        lb.append(l)
    lb = torch.stack(lb)
    assert la.shape == (K,) and la.dtype == torch.float32 and la.device.type == "cuda"
    assert torch.equal(la, lb), (la, lb)
    ta, tb = tensors_of(a), tensors_of(b)
    assert sorted(ta) == sorted(tb) and len(ta) == 6
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert a.opt_state["_lazy"]["step"] == b.opt_state["_lazy"]["step"] == first_step - 1 + K
    assert a.step == b.step == K
    assert bool(torch.isfinite(la).all())
    for k in PATHS:                            # and what anybody reads through the state (flushed) is the same too
        assert torch.equal(a.params["params"][k]["embedding"], b.params["params"][k]["embedding"]), k
    return a


# ------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("o", [1, 5, 64])
@pytest.mark.parametrize("step", [1, 1000])
def test_sampler_equals_the_numpy_restatement(dev, o, step):
    from esrecsys_amd import ops
    tracks, albums, artists = corpus()
    sampler = new_sampler(dev, o)
    want = negative_indices(SEED, step, o, T)
    idx, al, ar = sampler.sample(step)
    assert idx.dtype == al.dtype == ar.dtype == torch.int32 and idx.shape == al.shape == ar.shape == (o,)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(al.cpu().numpy(), albums[want]) and np.array_equal(ar.cpu().numpy(), artists[want])
    assert int(idx.max()) < T - 1 and int(idx.min()) >= 0          # the last track is never drawn
    assert torch.equal(sampler.indices(step), idx)
    x = sampler.fill({}, step)
    assert np.array_equal(x["neg_track"].cpu().numpy(), tracks[want]) and torch.equal(x["neg_album"], al)
    assert torch.equal(x["neg_artist"], ar)
    # another seed (low word only) and a two-track corpus (index 0 only)
    d_al, d_ar = sampler.albums, sampler.artists
    got = ops.spotify_sample_negatives(d_al, d_ar, 7, step, o)[0]
    assert np.array_equal(got.cpu().numpy(), negative_indices(7, step, o, T))
    assert not ops.spotify_sample_negatives(d_al[:2], d_ar[:2], SEED, step, o)[0].any()


def test_sampler_never_draws_the_last_track_over_many_steps(dev):
    sampler = new_sampler(dev, 64)
    seen = torch.zeros(T, dtype=torch.bool, device=dev)
    for step in range(1, 33):
        seen[sampler.indices(step).long()] = True
    assert bool(seen[:T - 1].all()) and not bool(seen[T - 1])


# ------------------------------------------------------------------------------------------------------ assembly
@pytest.mark.parametrize("n,o,K,first_step", [(5, 64, 9, 1), (1, 1, 9, 1000), (5, 5, 2, 1000), (1, 5, 1, 1), (5, 1, 3, 1)])
def test_group_call_assembles_the_lists_and_reports_the_indices(dev, n, o, K, first_step):
    """esr_spotify_train_steps through ops: neg_index [K, o] equals the restatement, and step j's block of the workspace
    holds occurrence_ids of playlist j with the sampler's negatives of step first_step + j."""
    from esrecsys_amd import _lib, ops
    F = 4
    xs = playlists(n, K)
    sampler = new_sampler(dev, o)
    state = new_state(dev, F, first_step)
    raw, tr = state.raw_params["params"], state.opt_state["trace"]["params"]
    lz = state.opt_state["_lazy"]
    lens = np.array(LENS[K], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    up = lambda key, shape: torch.from_numpy(np.concatenate([x[key] for x in xs]).astype(np.int32)).to(dev).view(shape)  # noqa: E731
    nbytes = _lib.load().esr_spotify_train_steps_workspace_bytes(n, int(lens.max()), o, F, K, int(off[-1]))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    neg_index = torch.full((K, o), -1, dtype=torch.int32, device=dev)
    losses = ops.spotify_train_steps(
        raw["album_embed"]["embedding"], tr["album_embed"]["embedding"], lz["last"][PATHS["album_embed"]],
        raw["artist_embed"]["embedding"], tr["artist_embed"]["embedding"], lz["last"][PATHS["artist_embed"]],
        up("album_context", (K, n)), up("artist_context", (K, n)), up("next_album", (-1,)), up("next_artist", (-1,)), off,
        torch.from_numpy(off).to(dev), sampler.albums, sampler.artists, SEED, first_step, o, REG, LR, MOM,
        neg_index=neg_index, workspace=ws)
    assert losses.shape == (K,) and bool(torch.isfinite(losses).all())
    want_idx = np.stack([negative_indices(SEED, first_step + j, o, T) for j in range(K)])
    assert np.array_equal(neg_index.cpu().numpy(), want_idx)
    assert want_idx.max() < T - 1
    lists = ws.view(torch.int32).cpu().numpy()
    starts = list_starts(n, off, o)
    assert np.array_equal(starts, ops.spotify_list_starts(n, off, o))
    bound = state.apply_fn(state.raw_params, method=lambda m: m)
    for j, x in enumerate(xs):
        al, ar, n_, m_, o_ = bound.occurrence_ids(*(sampler.fill(dict(x), first_step + j)[k] for k in (
            "album_context", "artist_context", "next_album", "next_artist", "neg_album", "neg_artist")))
        R = n + int(lens[j]) + o
        assert (n_, m_, o_) == (n, int(lens[j]), o) and al.numel() == R
        assert starts[j] % 64 == 0
        assert np.array_equal(lists[starts[j]:starts[j] + R], al.cpu().numpy()), j
        assert np.array_equal(lists[starts[j] + R:starts[j] + 2 * R], ar.cpu().numpy()), j
        f = with_negatives(x, first_step + j, o)                     # and the same from host arrays alone
        assert np.array_equal(al.cpu().numpy(), np.concatenate([f["album_context"], f["next_album"], f["neg_album"]]))


# ------------------------------------------------------------------------------------------------------ group = loop
@pytest.mark.parametrize("first_step", [1, 1000])
@pytest.mark.parametrize("K", [1, 2, 9])
@pytest.mark.parametrize("o", [1, 5, 64])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("F", [4, 32])
def test_group_equals_the_loop_bit_for_bit(dev, F, n, o, K, first_step):
    group_vs_loop(dev, F, n, o, K, first_step, group=64)


@pytest.mark.parametrize("group", [1, 4, 8])
@pytest.mark.parametrize("F,n,o,first_step", [(4, 1, 1, 1), (32, 5, 64, 1000), (32, 5, 5, 1)])
def test_group_boundary_mid_run(dev, F, n, o, first_step, group):
    """group < num_steps: 9 playlists as 9 x 1, 4 + 4 + 1 and 8 + 1 library calls"""
    group_vs_loop(dev, F, n, o, 9, first_step, group=group)


def test_the_playlists_share_rows_and_let_rows_rest():
    """(host only) what the cases above rely on: consecutive steps share rows, and with few negatives rows rest and return"""
    for n in (1, 5):
        for first_step in (1, 1000):
            assert rows_rest_and_return(playlists(n, 9), first_step, 1), (n, first_step)
    xs = playlists(5, 9)
    for a, b in zip(xs, xs[1:]):
        rows = lambda x: set((np.concatenate([x["album_context"], x["next_album"]]) % ROWS).tolist())  # noqa: E731
        assert rows(a) & rows(b)


def test_group_equals_the_loop_with_the_catch_up_launch(dev):
    """ESR_SPOTIFY_CATCHUP=launch (the catch-up as its own launch in front of every step), set in a fresh child process:
    the library reads the switch per call, the child never sees the default."""
    code = ("import sys; sys.path.insert(0, %r); import torch; import test_gpu_spotify_train_steps as t; "
            "dev = torch.device('cuda', 0); t.group_vs_loop(dev, 32, 5, 64, 9, 1, 4); t.group_vs_loop(dev, 4, 1, 1, 9, 1000, 64); "
            "print('GROUP_EQUALS_LOOP')" % os.path.join(ROOT, "tests"))
    env = dict(os.environ, ESR_SPOTIFY_CATCHUP="launch")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GROUP_EQUALS_LOOP" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------------------ oracle
def test_three_steps_against_the_fp64_oracle(dev, monkeypatch):
    """three steps of one group call at F = 4 against oracle/spotify.py's dense gradients and momentum update, fed the
    sampler's negatives (the oracle hashes albums with its MAX_ALBUMS: set to this world's 7 rows)"""
    from esrecsys_amd.spotify.train_spotify import train_steps
    monkeypatch.setattr(o_sp, "MAX_ALBUMS", ROWS)
    n, o, K = 5, 5, 3
    xs = playlists(n, K)
    state = new_state(dev, 4)
    at = state.raw_params["params"]["album_embed"]["embedding"].cpu().numpy().astype(F64)
    rt = state.raw_params["params"]["artist_embed"]["embedding"].cpu().numpy().astype(F64)
    ta, tr = np.zeros_like(at), np.zeros_like(rt)
    state, losses = train_steps(state, iter(xs), K, REG, new_sampler(dev, o))
    losses = losses.cpu().numpy()
    for j, x in enumerate(xs):
        el, ga, gr = o_sp.dense_grads(at, rt, with_negatives(x, 1 + j, o), REG)
        at, ta = o_sp.sgd_momentum_update(at, ta, ga, LR, MOM, F64)
        rt, tr = o_sp.sgd_momentum_update(rt, tr, gr, LR, MOM, F64)
        print("step %d: loss %.9g oracle %.9g rel %.3g" % (j, losses[j], el, abs(losses[j] - el) / abs(el)))
        assert abs(float(losses[j]) - el) <= TOL * abs(el), j
    assert state.step == K
    p, t = state.params["params"], state.opt_state["trace"]["params"]
    errs = [rel_err(p["album_embed"]["embedding"].cpu().numpy(), at), rel_err(p["artist_embed"]["embedding"].cpu().numpy(), rt),
            rel_err(t["album_embed"]["embedding"].cpu().numpy(), ta), rel_err(t["artist_embed"]["embedding"].cpu().numpy(), tr)]
    print("rel_err album, artist, album trace, artist trace:", errs)
    assert max(errs) <= TOL


# ------------------------------------------------------------------------------------------------------ fallback, errors
def test_a_dense_sgd_state_takes_the_per_playlist_loop(dev):
    """optim.sgd(lr, momentum, lazy=False) is not on the one-call path: train_steps gives what its own loop gives"""
    from esrecsys_amd.spotify.train_spotify import train_step, train_steps
    n, o, K = 5, 5, 3
    xs = playlists(n, K)
    sampler = new_sampler(dev, o)
    a, b = new_state(dev, 4, lazy=False), new_state(dev, 4, lazy=False)
    a, la = train_steps(a, iter([dict(x) for x in xs]), K, REG, sampler)
    lb = []
    for j, x in enumerate(xs):
        b, l = train_step(b, sampler.fill(dict(x), 1 + j), REG)
        lb.append(l)
    assert torch.equal(la, torch.stack(lb)) and la.shape == (K,) and a.step == b.step == K
    ta, tb = tensors_of(a), tensors_of(b)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert all("neg_album" not in x for x in xs)                    # the caller's dicts are left alone


def test_errors(dev):
    from esrecsys_amd.spotify.train_spotify import NegativeSampler, train_steps
    tracks, albums, artists = corpus()
    sampler = new_sampler(dev, 5)
    xs = playlists(5, 2)
    short = dict(xs[1], album_context=xs[1]["album_context"][:4], artist_context=xs[1]["artist_context"][:4])
    with pytest.raises(ValueError, match="one context length"):
        train_steps(new_state(dev, 4), iter([xs[0], short]), 2, REG, sampler)
    empty = dict(xs[1], next_album=xs[1]["next_album"][:0], next_artist=xs[1]["next_artist"][:0])
    with pytest.raises(ValueError, match="non-empty next list"):
        train_steps(new_state(dev, 4), iter([xs[0], empty]), 2, REG, sampler)
    bad = dict(xs[1], next_artist=np.full_like(xs[1]["next_artist"], N_ART))
    with pytest.raises(IndexError, match=r"\[0, %d\)" % N_ART):
        train_steps(new_state(dev, 4), iter([xs[0], bad]), 2, REG, sampler)
    neg = dict(xs[1], artist_context=np.full_like(xs[1]["artist_context"], -1))
    with pytest.raises(IndexError):
        train_steps(new_state(dev, 4), iter([xs[0], neg]), 2, REG, sampler)
    wrong = artists.copy()
    wrong[3] = N_ART
    with pytest.raises(IndexError, match="corpus"):
        NegativeSampler(tracks, albums, wrong, 5, SEED, N_ART, dev)
    with pytest.raises(ValueError, match="T >= 2"):
        NegativeSampler(tracks[:1], albums[:1], artists[:1], 5, SEED, N_ART, dev)
    with pytest.raises(ValueError, match="differ in length"):
        NegativeSampler(tracks, albums[:5], artists, 5, SEED, N_ART, dev)
    # a sampler whose corpus may name artists beyond the state's table is refused before anything is launched
    wide = NegativeSampler(tracks, albums, artists, 5, SEED, N_ART + 1, dev)
    with pytest.raises(IndexError, match="artist table"):
        train_steps(new_state(dev, 4), iter(xs), 2, REG, wide)
    # nothing above moved a state: a good call still starts at step 1
    state, losses = train_steps(new_state(dev, 4), iter(xs), 2, REG, sampler)
    assert state.opt_state["_lazy"]["step"] == 2 and losses.shape == (2,)

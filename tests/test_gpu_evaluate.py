"""GPU: esrecsys_amd.evaluate (esr_eval.hip) against the NumPy oracle of tests/_evaluate_ref.py, BIT FOR BIT: integers
equal, float32 arrays equal as uint32 views.  List widths around the wave and workgroup sizes and at the cap, lengths
0 / 1 / width - 1 / width and none, truth sets from empty to the cap, duplicate / huge / consecutive / colliding truth
ids, all-hit, no-hit and repeated lists under both repeat rules, the grid-stride loop, the refusals, split_holdout, the
whole pipeline at toy size and the Spotify model's eval."""
import numpy as np
import pytest
import torch

import _evaluate_ref as ref

pytestmark = pytest.mark.gpu
FLOATS = ("precision", "recall", "rr", "ap", "ndcg")
GRID_CAP = 256 * 8   # esr_common.h kMaxGrid: the launcher's grid; more queries go round the grid-stride loop


def N(t):
    return t.detach().cpu().numpy()


def assert_equals_oracle(got, want):
    for name in ("hits", "first_hit", "valid"):
        g = N(getattr(got, name))
        assert g.dtype == np.int32 and np.array_equal(g, want[name]), name
    for name in FLOATS:
        g = getattr(got, name)
        if want[name] is None:
            assert g is None, name
            continue
        g = N(g)
        assert g.dtype == np.float32 and g.shape == want[name].shape, name
        bad = np.flatnonzero((g.view(np.uint32) != want[name].view(np.uint32)).reshape(-1))
        assert bad.size == 0, (name, bad[:5], g.reshape(-1)[bad[:5]], want[name].reshape(-1)[bad[:5]])


def run(dev, rec, lengths, truth, off, ks, **kw):
    from esrecsys_amd.evaluate import ranking_metrics
    rec, truth, off = np.asarray(rec, np.int32), np.asarray(truth, np.int32), np.asarray(off, np.int64)
    d_len = None if lengths is None else torch.from_numpy(np.asarray(lengths, np.int32)).to(dev)
    got = ranking_metrics(torch.from_numpy(rec).to(dev), d_len, torch.from_numpy(truth).to(dev),
                          torch.from_numpy(off).to(dev), ks=ks, **kw)
    want = ref.ranking_metrics(rec, lengths, truth, off, ks, **kw)
    assert_equals_oracle(got, want)
    return got, want


def csr(sets):
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(s) for s in sets], out=off[1:])
    return (np.concatenate([np.asarray(s, np.int64) for s in sets]) if sets else np.zeros(0)).astype(np.int32), off


def cutoffs(width):
    """eight cutoffs with 1, the width and one above it"""
    ks = {k for k in (1, 2, 3, width // 2, width - 1, width, width + 1) if k >= 1}
    extra = width + 2
    while len(ks) < 8:
        ks.add(extra)
        extra += 1
    return tuple(sorted(ks))


@pytest.mark.parametrize("width", [1, 63, 64, 65, 500, 1024, 4096])
def test_widths_lengths_and_cutoffs(dev, width):
    rng = np.random.default_rng(width)
    universe = 3 * width + 10
    nq = 6
    rec = np.stack([rng.permutation(universe)[:width] for _ in range(nq)]).astype(np.int32)
    rec[1, width // 2:] = rec[1, 0]                                  # a list that repeats its head
    lengths = np.array([0, 1, max(width - 1, 0), width, width, width // 2], np.int32)
    for q in range(nq):
        rec[q, lengths[q]:] = -1                                     # padded as recommend pads
    truth, off = csr([rng.permutation(universe)[:n] for n in (width, 1, min(width, 70), min(universe // 2, 4096), 3, 40)])
    ks = cutoffs(width)
    assert len(ks) == 8 and 1 in ks and width in ks and width + 1 in ks
    got, want = run(dev, rec, lengths, truth, off, ks)
    assert want["hits"].max() > 0
    # null lengths: the padding is read, and -1 is nobody's truth id
    run(dev, rec, None, truth, off, ks)
    full = np.stack([rng.permutation(universe)[:width] for _ in range(nq)]).astype(np.int32)
    run(dev, full, None, truth, off, ks[-3:])
    run(dev, full, None, truth, off, (1,))
    # a view with a row pitch above its width takes the same path
    from esrecsys_amd.evaluate import ranking_metrics
    wide = torch.full((nq, width + 3), 7, dtype=torch.int32, device=dev)
    wide[:, :width] = torch.from_numpy(full).to(dev)
    view = ranking_metrics(wide[:, :width], None, torch.from_numpy(truth).to(dev), torch.from_numpy(off).to(dev), ks=ks)
    assert_equals_oracle(view, ref.ranking_metrics(full, None, truth, off, ks))


@pytest.mark.parametrize("nq", [1, 3, 257])
@pytest.mark.parametrize("n_truth", [0, 1, 2, 63, 64, 65, 4096])
def test_truth_lengths(dev, nq, n_truth):
    rng = np.random.default_rng(1000 * nq + n_truth)
    width, universe = 70, 3 * max(n_truth, 70)
    base = rng.permutation(universe)
    sets = [np.roll(base, 17 * q)[:n_truth] for q in range(nq)]      # distinct ids, another set per query
    truth, off = csr(sets)
    rec = rng.integers(0, universe, (nq, width)).astype(np.int32)    # with repeats inside a list
    lengths = rng.integers(0, width + 1, nq).astype(np.int32)
    for kw in ({}, {"truth_size": "listed"}, {"count_repeats": True}):
        got, want = run(dev, rec, lengths, truth, off, (1, 10, 70, 100), **kw)
    assert want["valid"].sum() == (nq if n_truth else 0)


def test_mixed_truth_lengths_in_one_call(dev):
    """every query sizes its own table: empty, tiny and cap-sized truth sets side by side"""
    rng = np.random.default_rng(5)
    sizes = [0, 4096, 1, 33, 0, 2, 4096, 64, 65, 500]
    truth, off = csr([rng.permutation(20_000)[:n] for n in sizes])
    rec = rng.integers(0, 20_000, (len(sizes), 300)).astype(np.int32)
    got, want = run(dev, rec, None, truth, off, (5, 50, 300))
    assert want["valid"].tolist() == [int(n > 0) for n in sizes]


def test_truth_contents(dev):
    rng = np.random.default_rng(6)
    big = 2 ** 31 - 2
    sets = [
        [5, 5, 5, 9, 9, 11],                                         # duplicates: 3 distinct, 6 listed
        [big, big - 1, 0, big, 12],                                  # the largest ids
        np.arange(1000, 1000 + 4096),                                # the cap, consecutive
        np.arange(4096, dtype=np.int64) * 8192,                      # the cap; a low-bit hash would chain all of these
        np.repeat(np.arange(50), 100),                               # 5000 listed, 50 distinct: above the cap as listed
    ]
    truth, off = csr(sets)
    rec = np.stack([
        np.resize([9, 4, 5, 5, 11, 3], 64), np.resize([1, big, 12, big - 1, 7, big], 64),
        rng.integers(0, 6000, 64), rng.integers(0, 4096, 64) * 8192 + (rng.random(64) < 0.3), rng.integers(0, 100, 64),
    ]).astype(np.int32)
    for kw in ({}, {"truth_size": "listed"}, {"count_repeats": True, "truth_size": "listed"}):
        got, want = run(dev, rec, None, truth, off, (1, 6, 64), **kw)
    assert want["hits"][:, -1].min() > 0


@pytest.mark.parametrize("count_repeats", [False, True])
def test_hit_patterns(dev, count_repeats):
    width = 130
    truth_ids = np.arange(0, 2 * width, 2)
    rec = np.stack([
        truth_ids[:width],                                           # every position hits
        truth_ids[:width] + 1,                                       # none does
        np.resize(truth_ids[:7], width),                             # seven ids over and over
        np.resize([1, 3, 4, 4, 5], width),                           # one truth id, repeated, first at rank 3
    ]).astype(np.int32)
    truth, off = csr([truth_ids] * 4)
    got, want = run(dev, rec, None, truth, off, (1, 7, 64, 65, 130, 200), count_repeats=count_repeats)
    assert want["hits"][:, 4].tolist() == ([130, 0, 130, 52] if count_repeats else [130, 0, 7, 1])
    assert want["first_hit"].tolist() == [1, 0, 1, 3]


def test_more_queries_than_the_grid(dev):
    nq = GRID_CAP + 3
    rng = np.random.default_rng(8)
    rec = rng.integers(0, 12, (nq, 4)).astype(np.int32)
    truth = rng.integers(0, 12, 2 * nq).astype(np.int32)
    rec[GRID_CAP:, 1] = truth[2 * GRID_CAP::2]                       # the queries of the second round hit at rank 2
    got, want = run(dev, rec, None, truth, np.arange(nq + 1) * 2, (1, 4))
    assert want["hits"][GRID_CAP:, 1].min() > 0 and 0 < want["hits"][:, 1].mean() < 4


def test_refusals(dev):
    """Argument errors raise before any launch; a negative truth id is seen by the kernel (its failure word), as the
    pair-table builders see theirs, and raises after it."""
    from esrecsys_amd.evaluate import EvaluationError, ranking_metrics
    rec = torch.zeros((2, 8), dtype=torch.int32, device=dev)
    small, off = torch.tensor([1, 2, 3], dtype=torch.int32, device=dev), torch.tensor([0, 1, 3], device=dev)
    many = torch.arange(4097 + 1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match=r"query 1 has 4097 distinct truth ids"):
        ranking_metrics(rec, None, many, torch.tensor([0, 1, 4098], device=dev))
    ranking_metrics(rec, None, many[:4097], torch.tensor([0, 1, 4097], device=dev))          # 4096 are taken
    with pytest.raises(ValueError, match="width 4097"):
        ranking_metrics(torch.zeros((2, 4097), dtype=torch.int32, device=dev), None, small, off)
    with pytest.raises(ValueError, match="ascending"):
        ranking_metrics(rec, None, small, off, ks=(10, 100, 50))
    with pytest.raises(ValueError, match="9 cutoffs"):
        ranking_metrics(rec, None, small, off, ks=tuple(range(1, 10)))
    with pytest.raises(ValueError, match="3 truth sets for 2 lists"):
        ranking_metrics(rec, None, small, torch.tensor([0, 1, 2, 3], device=dev))
    with pytest.raises(ValueError, match="1 lengths for 2 lists"):
        ranking_metrics(rec, torch.zeros(1, dtype=torch.int32, device=dev), small, off)
    with pytest.raises(ValueError, match="rise from 0"):
        ranking_metrics(rec, None, small, torch.tensor([0, 1, 2], device=dev))
    with pytest.raises(TypeError, match="no CPU fallback"):
        ranking_metrics(rec.cpu(), None, small, off)
    with pytest.raises(EvaluationError, match="negative truth id"):
        ranking_metrics(rec, None, torch.tensor([1, -2, 3], dtype=torch.int32, device=dev), off)
    empty = ranking_metrics(rec[:0], None, small[:0], off[:1])
    assert empty.hits.shape == (0, 3) and empty.mean()["n_valid"] == 0


@pytest.mark.parametrize("mode", ["first", "last"])
def test_split_holdout_on_the_device(dev, mode):
    from esrecsys_amd.evaluate import split_holdout
    rng = np.random.default_rng(3)
    lengths = np.array([10, 9, 0, 11, 200, 10, 3, 9, 10, 57])       # exactly min_length, one below it, empty
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ids = rng.integers(0, 2 ** 31 - 1, int(off[-1])).astype(np.int32)
    got = split_holdout(torch.from_numpy(ids).to(dev), torch.from_numpy(off).to(dev), mode=mode)
    want = ref.split_holdout(ids, off, mode=mode)
    assert want[4].tolist() == [0, 3, 4, 5, 8, 9]
    for g, w in zip(got, want):
        assert g.device.type == "cuda" and g.dtype == torch.from_numpy(w).dtype and np.array_equal(N(g), w)
    none = split_holdout(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert [t.numel() for t in none] == [0, 1, 0, 1, 0] and all(t.device.type == "cuda" for t in none)


def test_pipeline_at_toy_size(dev):
    """split_holdout -> DiceBuilder -> neighbours -> recommend -> ranking_metrics on 300 documents over 50 ids"""
    from esrecsys_amd.evaluate import ranking_metrics, split_holdout
    from esrecsys_amd.wikipedia.make_dice import DiceBuilder
    from esrecsys_amd.wikipedia.neighbours import neighbours, recommend
    rng = np.random.default_rng(12)
    lengths = rng.integers(6, 25, 300)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    group = np.repeat(rng.integers(0, 5, 300), lengths)              # documents draw from one of five groups of ten ids
    ids = (group * 10 + rng.integers(0, 10, int(off[-1]))).astype(np.int32)
    ctx, c_off, truth, t_off, kept = split_holdout(torch.from_numpy(ids).to(dev), torch.from_numpy(off).to(dev))
    assert 0 < kept.numel() < 300
    b = DiceBuilder(capacity=1 << 12, device=dev).add(ctx, c_off)
    index, other, count = b.finalize()
    table = neighbours(index, other, count, *b.doc_frequency(), k=8)
    rec_ids, _, rec_lengths = recommend(table, ctx, c_off, k=20)
    ks = (1, 5, 20)
    got = ranking_metrics(rec_ids, rec_lengths, truth, t_off, ks=ks)
    want = ref.ranking_metrics(N(rec_ids), N(rec_lengths), N(truth), N(t_off), ks)
    assert_equals_oracle(got, want)
    mean, want_mean = got.mean(), ref.mean(want)
    assert mean["n_valid"] == want_mean["n_valid"] == kept.numel()
    for name in FLOATS:
        assert mean[name].dtype == np.float64 and mean[name].shape == (3,)
        assert np.all(np.abs(mean[name] - want_mean[name]) <= 1e-15 * np.abs(want_mean[name])), name
    assert mean["recall"][2] > mean["recall"][0] > 0                 # the groups are learnt: this is not noise


def _spotify_world(dev, P, T=200_003, n_art=4000, seed=4):
    """the small model of tests/test_gpu_spotify_eval_batch.py and its ragged next lists"""
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.spotify.models import SpotifyModel
    from esrecsys_amd.spotify.train_spotify import all_track_top_k_batch
    rng = np.random.default_rng(seed)
    model = SpotifyModel(feature_size=32, device=dev, num_artists=n_art)
    all_tracks = (np.arange(T, dtype=np.int64) * 7 + 3).astype(np.int32)      # track ids are not positions
    all_albums, all_artists = rng.integers(0, 100_000, T).astype(np.int32), rng.integers(0, n_art, T).astype(np.int32)
    state = TrainState.create(apply_fn=model.apply, params=model.init(1701), tx=optim.sgd(1e-3, 0.98))
    ys = []
    for p in range(P):
        pick = rng.integers(0, T, 5)
        ys.append({"album_context": all_albums[pick], "artist_context": all_artists[pick]})
    _, tops = all_track_top_k_batch(state, ys, all_albums, all_artists)
    for p, y in enumerate(ys):
        top = N(tops[p]).astype(np.int64)
        m = int(rng.integers(1, 251)) if p % 3 else int(rng.integers(1, 4))
        nx = np.concatenate([rng.choice(top, int(rng.integers(0, min(m, 40) + 1))), rng.integers(0, T, m)])[:m]
        if m > 2:
            nx[-1] = nx[0]                                                   # a repeated next track
        y["next_track"], y["next_artist"] = all_tracks[nx], all_artists[nx]
    return state, ys, all_tracks, all_albums, all_artists, tops


def test_spotify_reference_metric_and_eval_metrics(dev):
    from esrecsys_amd.evaluate import ranking_metrics
    from esrecsys_amd.spotify.train_spotify import eval_batch, eval_metrics
    state, ys, all_tracks, all_albums, all_artists, tops = _spotify_world(dev, 30)
    tracks = torch.from_numpy(all_tracks).to(dev)[tops.long()]
    truth, off = csr([y["next_track"] for y in ys])
    # the reference's own metric, isin(top, next).sum() / numel(next): repeats counted, the listed size
    m = ranking_metrics(tracks, None, truth, off, ks=(500,), count_repeats=True, truth_size="listed")
    inv = torch.from_numpy(np.float32(1.0) / np.diff(off).astype(np.float32)).to(dev)
    want = eval_batch(state, ys, all_tracks, all_albums, all_artists)
    assert torch.equal(m.hits[:, 0].float() * inv, want[:, 0]) and float(want[:, 0].max()) > 0
    assert_equals_oracle(m, ref.ranking_metrics(N(tracks), None, truth, off, (500,), count_repeats=True,
                                                truth_size="listed"))
    got = eval_metrics(state, ys, all_tracks, all_albums, all_artists)
    assert got.ks == (10, 100, 500)
    assert_equals_oracle(got, ref.ranking_metrics(N(tracks), None, truth, off, (10, 100, 500)))
    short = eval_metrics(state, ys, all_tracks, all_albums, all_artists, ks=(10,))
    assert torch.equal(short.hits[:, 0], got.hits[:, 0]) and torch.equal(short.ndcg[:, 0], got.ndcg[:, 0])

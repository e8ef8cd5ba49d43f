"""Training / eval steps of the Spotify model -- drop-in for ``spotify/train_spotify.py:77-150``.

``train_step(state, x, regularization) -> (new_state, loss)`` and ``eval_step(state, y, all_tracks, all_albums,
all_artists) -> metrics[2]`` keep the reference's signatures; ``x`` / ``y`` are the reference's feature dicts.
``eval_batch`` / ``eval_steps`` score many playlists per library call and return what the per-playlist loop returns.
The optimizer of the reference is ``optax.sgd(learning_rate, momentum)`` = ``esrecsys_amd.optim.sgd(lr, momentum)``.
"""
import numpy as np
import torch

from .. import ops
from ..train_state import RowGrads

FLAGS = dict(num_negatives=64, learning_rate=1e-3, momentum=0.98, regularization=10.0, feature_size=32,
             log_every_steps=1000, eval_every_steps=10000, eval_steps=1000, checkpoint_every_steps=100000,
             max_steps=2000000)  # train_spotify.py:60-70
TOP_K = 500  # train_spotify.py:120


def _model_of(state):
    fn = state.apply_fn
    return getattr(fn, "__self__", None)


def train_step(state, x, regularization):
    """train_spotify.py:77-111: value_and_grad of the six-term loss, then apply_gradients."""
    model = _model_of(state)
    raw = state.raw_params  # (the hot loop: state.params would bring EVERY row of the lazily updated tables up to date)
    p = raw["params"]
    at, rt = p["album_embed"]["embedding"], p["artist_embed"]["embedding"]
    bound = model.apply(raw, method=lambda m: m)  # bind the tables to read the occurrence ids
    al, ar, n, m, o = bound.occurrence_ids(x["album_context"], x["artist_context"], x["next_album"], x["next_artist"],
                                           x["neg_album"], x["neg_artist"])
    tx = state.tx
    if getattr(tx, "lazy", False) and hasattr(tx, "_lazy_state") and at.is_cuda and at.shape[1] == rt.shape[1]:
        # the reference's optimizer (optax.sgd(lr, momentum), train_spotify.py:238-241) in its lazy form: the whole step --
        # catch-up of the playlist's rows, loss, gradient rows, one sort, the momentum step on the touched rows of both
        # tables -- is ONE library call (eight launches; issued from Python the step was host-bound)
        lz = tx._lazy_state(raw, state.opt_state)
        lz["step"] += 1
        tr = state.opt_state["trace"]["params"]
        loss = ops.spotify_train_step(at, tr["album_embed"]["embedding"], lz["last"][("params", "album_embed", "embedding")],
                                      rt, tr["artist_embed"]["embedding"],
                                      lz["last"][("params", "artist_embed", "embedding")], al, ar, n, m, o, regularization,
                                      lz["step"], tx.lr, tx.momentum)
        lz["dirty"] = True
        return state.replace(step=state.step + 1), loss.reshape(())
    if hasattr(state.tx, "prepare"):
        # optax.sgd(lr, momentum) in its lazy form: the rows this playlist reads are brought up to date here (albums are
        # hashed into the table: row = album mod rows, spotify/models.py:37-41), nobody else's are touched
        state.tx.prepare(raw, state.opt_state, [(("params", "album_embed", "embedding"), al, at.shape[0]),
                                                (("params", "artist_embed", "embedding"), ar, 0)])
    loss, album_rows, ga, gr = ops.spotify_fwd_bwd(at, rt, al, ar, n, m, o, regularization)
    grads = {"params": {"album_embed": {"embedding": RowGrads([album_rows], ga, at.shape)},
                        "artist_embed": {"embedding": RowGrads([ar], gr, rt.shape)}}}
    return state.apply_gradients(grads=grads), loss.reshape(())


def all_track_top_k(state, y, all_albums, all_artists, k=TOP_K, segments=64):
    """jax.lax.top_k(all_affinity, 500) over the whole corpus (train_spotify.py:119-120): (scores[k], indices[k]).
    Two levels through the batched select kernel: top-k of `segments` slices, then of their union."""
    p = state.params["params"]
    at, rt = p["album_embed"]["embedding"], p["artist_embed"]["embedding"]
    dev = at.device
    ca, cr = ops.as_ids(y["album_context"], dev).reshape(-1), ops.as_ids(y["artist_context"], dev).reshape(-1)
    aa, rr = ops.as_ids(all_albums, dev).reshape(-1), ops.as_ids(all_artists, dev).reshape(-1)
    aff = ops.spotify_affinity_all(at, rt, ca, cr, aa, rr)
    T = aff.numel()
    k = min(k, T)
    seg = max(k, -(-T // segments))
    rows = -(-T // seg)
    pad = rows * seg - T
    idx = torch.arange(rows * seg, dtype=torch.int32, device=dev)
    if pad:
        aff = torch.cat([aff, torch.full((pad,), float("-inf"), device=dev)])
    s1, i1 = ops.topk_merge(aff.reshape(rows, seg), idx.reshape(rows, seg), k)
    s, i = ops.topk_merge(s1.reshape(1, -1), i1.reshape(1, -1), k)
    return s[0], i[0]


def eval_step(state, y, all_tracks, all_albums, all_artists):
    """train_spotify.py:113-131: recall of the next tracks / artists among the 500 best-scoring tracks."""
    dev = state.params["params"]["album_embed"]["embedding"].device
    _, top = all_track_top_k(state, y, all_albums, all_artists)
    tracks = ops.as_ids(all_tracks, dev).reshape(-1)[top.long()]
    artists = ops.as_ids(all_artists, dev).reshape(-1)[top.long()]
    nt, na = ops.as_ids(y["next_track"], dev).reshape(-1), ops.as_ids(y["next_artist"], dev).reshape(-1)
    tracks_recall = torch.isin(tracks, nt).sum().float() / nt.numel()
    artists_recall = torch.isin(artists, na).sum().float() / na.numel()
    return torch.stack([tracks_recall, artists_recall])


def _context_length(ys):
    """The common context length of a batch of playlists (ValueError for an empty batch or mixed lengths)."""
    if len(ys) == 0:
        raise ValueError("an empty batch of playlists")
    size = lambda v: v.numel() if isinstance(v, torch.Tensor) else int(np.size(v))  # noqa: E731
    lens = {size(y["album_context"]) for y in ys} | {size(y["artist_context"]) for y in ys}
    if len(lens) != 1:
        raise ValueError("the playlists of one batch must have one context length, got %s" % sorted(lens))
    return lens.pop()


def _stack_ids(values, dev):
    """[P, n] int32 on `dev` from P id lists: one upload when they are host arrays."""
    if any(isinstance(v, torch.Tensor) for v in values):
        return torch.stack([ops.as_ids(v, dev).reshape(-1) for v in values])
    return ops.as_ids(np.stack([np.asarray(v).reshape(-1) for v in values]), dev)


def all_track_top_k_batch(state, ys, all_albums, all_artists, k=TOP_K):
    """all_track_top_k for a batch of playlists (the reference's feature dicts, one context length): (scores [P, k],
    indices [P, k]), row p bit-identical to all_track_top_k(state, ys[p], ...).  One library call scores the corpus
    for all of them (esr_spotify_topk_batch); the tables are read through state.params once."""
    _context_length(ys)
    p = state.params["params"]
    at, rt = p["album_embed"]["embedding"], p["artist_embed"]["embedding"]
    dev = at.device
    ca, cr = _stack_ids([y["album_context"] for y in ys], dev), _stack_ids([y["artist_context"] for y in ys], dev)
    aa, rr = ops.as_ids(all_albums, dev).reshape(-1), ops.as_ids(all_artists, dev).reshape(-1)
    return ops.spotify_topk_batch(at, rt, ca, cr, aa, rr, min(k, aa.numel()))


_NO_ID = 1 << 40  # pads the ragged next lists: above every int32 id


def _recall(top_ids, nexts, dev):
    """Per row: how many of top_ids [P, k] are in that row's next list, over the list's length (eval_step's
    isin(...).sum().float() / numel, row by row)."""
    if any(isinstance(v, torch.Tensor) for v in nexts):
        rows = [ops.as_ids(v, dev).reshape(-1) for v in nexts]
        lens = [r.numel() for r in rows]
        L = max(lens)
        # one scatter of all the lists (a copy per row was a launch per playlist)
        at_row = np.repeat(np.arange(len(rows)), lens)
        at_col = np.arange(at_row.size) - np.repeat(np.cumsum(lens) - lens, lens)
        pad = torch.full((len(rows), L), _NO_ID, dtype=torch.int64, device=dev)
        pad[torch.from_numpy(at_row).to(dev), torch.from_numpy(at_col).to(dev)] = torch.cat(rows).long()
    else:
        rows = [np.asarray(v).reshape(-1) for v in nexts]
        L = max(r.size for r in rows)
        pad = np.full((len(rows), L), _NO_ID, dtype=np.int64)
        for i, r in enumerate(rows):
            pad[i, :r.size] = r
        pad = torch.from_numpy(pad).to(dev)
        lens = [r.size for r in rows]
    pad = pad.sort(dim=1).values
    ids = top_ids.long()
    pos = torch.searchsorted(pad, ids).clamp_(max=L - 1)
    hits = (pad.gather(1, pos) == ids).sum(dim=1)
    # eval_step's `count.float() / numel` divides a device tensor by a host scalar, which torch computes as
    # count * (1 / numel) with the reciprocal rounded to float32 on the host: the same here, row by row
    inv = torch.from_numpy(np.float32(1.0) / np.asarray(lens, dtype=np.float32)).to(dev)
    return hits.float() * inv


def eval_batch(state, ys, all_tracks, all_albums, all_artists):
    """eval_step for a batch of playlists: metrics [P, 2], row p bit-identical to eval_step(state, ys[p], ...)."""
    _, top = all_track_top_k_batch(state, ys, all_albums, all_artists)
    dev = top.device
    top = top.long()
    tracks = ops.as_ids(all_tracks, dev).reshape(-1)[top]
    artists = ops.as_ids(all_artists, dev).reshape(-1)[top]
    return torch.stack([_recall(tracks, [y["next_track"] for y in ys], dev),
                        _recall(artists, [y["next_artist"] for y in ys], dev)], dim=1)


def eval_metrics(state, ys, all_tracks, all_albums, all_artists, ks=(10, 100, 500)):
    """The ranking metrics (``esrecsys_amd.evaluate.RankingMetrics``: hits, precision, recall, reciprocal rank, average
    precision and nDCG at every cutoff of `ks`) of the track ids behind all_track_top_k_batch against each playlist's
    ``next_track`` list, taken as a set.  eval_batch's track recall is the ``count_repeats=True, truth_size="listed"`` form
    of the same kernel at ks=(500,)."""
    from ..evaluate import ranking_metrics
    _, top = all_track_top_k_batch(state, ys, all_albums, all_artists, k=max(int(k) for k in ks))
    dev = top.device
    tracks = ops.as_ids(all_tracks, dev).reshape(-1)[top.long()]
    nexts = [_host_ids(y["next_track"]) for y in ys]
    offsets = np.zeros(len(nexts) + 1, np.int64)
    np.cumsum([v.size for v in nexts], out=offsets[1:])
    return ranking_metrics(tracks, None, np.concatenate(nexts).astype(np.int32), offsets, ks=ks)


def eval_steps(state, test_it, eval_steps, all_tracks, all_albums, all_artists, batch=256):
    """The eval of train_spotify.py:270-276: `eval_steps` playlists drawn from `test_it`, their eval_step metrics summed
    in float32 in playlist order and divided by eval_steps -- bit for bit the reference's loop -- scored `batch`
    playlists per call.  Returns the average metrics [2] (float32, on the tables' device)."""
    if eval_steps < 1 or batch < 1:
        raise ValueError("eval_steps and batch must be >= 1, got %d and %d" % (eval_steps, batch))
    s = np.zeros(2, np.float32)
    left = eval_steps
    while left:
        ys = [next(test_it) for _ in range(min(batch, left))]
        left -= len(ys)
        for m in eval_batch(state, ys, all_tracks, all_albums, all_artists).cpu().numpy():
            s = s + m                      # sequential, as the loop's sum_metrics = sum_metrics + eval_metrics
    dev = state.params["params"]["album_embed"]["embedding"].device
    return torch.from_numpy(s).to(dev) / eval_steps   # (the loop's division, by the same torch kernel)


def sample_negative(x, rng, num_negatives, all_tracks, all_albums, all_artists):
    """train_spotify.py:139-150.  `rng` is a numpy Generator (JAX's threefry stream is not reproducible without
    JAX); like the reference, the upper bound is exclusive of the last track."""
    idx = rng.integers(0, len(all_tracks) - 1, num_negatives)
    x["neg_track"] = np.asarray(all_tracks)[idx]
    x["neg_album"] = np.asarray(all_albums)[idx]
    x["neg_artist"] = np.asarray(all_artists)[idx]
    return rng


def _host_ids(v):
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).reshape(-1)


class NegativeSampler:
    """sample_negative (train_spotify.py:139-150) on the device: the corpus is uploaded and validated ONCE, and the
    negatives of a step are a pure function of (seed, step) -- never of the model -- so a loop can draw them for many
    steps ahead (train_steps) and a restored run continues the same stream.

    Negative i of step s: word i & 3 of Philox4x32-10 (Random123) with counter (i >> 2, s, 0, 0) and key (seed & 0xffffffff,
    seed >> 32); track index = (word * (T - 1)) >> 32.  Like the reference the last track is never drawn; multiply-high is
    biased by at most (T - 1) / 2^32 relative (5.3e-4 at the reference's 2 262 292 tracks).  This is not JAX's threefry
    stream (which is not reproducible without JAX) and not sample_negative's NumPy stream.

    Raises ValueError for arrays of different lengths or fewer than two tracks, IndexError for an artist id outside
    [0, n_artists)."""

    def __init__(self, all_tracks, all_albums, all_artists, num_negatives, seed, n_artists, device):
        sizes = {int(v.numel()) if isinstance(v, torch.Tensor) else int(np.size(v))
                 for v in (all_tracks, all_albums, all_artists)}
        if len(sizes) != 1:
            raise ValueError("all_tracks, all_albums and all_artists differ in length: %s" % sorted(sizes))
        self.T = sizes.pop()
        if self.T < 2:
            raise ValueError("a corpus of %d track(s): negatives are drawn from all but the last, T >= 2 is required" % self.T)
        if int(num_negatives) < 1:
            raise ValueError("num_negatives must be >= 1, got %d" % num_negatives)
        self.num_negatives, self.seed, self.n_artists = int(num_negatives), int(seed) & (2 ** 64 - 1), int(n_artists)
        self.tracks = ops.as_ids(all_tracks, device).reshape(-1)
        self.albums = ops.as_ids(all_albums, device).reshape(-1)
        self.artists = ops.as_ids(all_artists, device).reshape(-1)
        lo, hi = int(self.artists.min()), int(self.artists.max())
        if lo < 0 or hi >= self.n_artists:
            raise IndexError("artist id out of range [0, %d) in the corpus: min %d max %d" % (self.n_artists, lo, hi))

    def sample(self, step):
        """(index, album, artist) of the step's negatives: device int32 [num_negatives] each."""
        return ops.spotify_sample_negatives(self.albums, self.artists, self.seed, step, self.num_negatives)

    def indices(self, step):
        return self.sample(step)[0]

    def fill(self, x, step):
        """The per-step counterpart of sample_negative: x's neg_track / neg_album / neg_artist as device tensors."""
        idx, x["neg_album"], x["neg_artist"] = self.sample(step)
        x["neg_track"] = self.tracks[idx.long()]
        return x


def _fused(state):
    """(album table, artist table) when train_step would take its one-call path for this state, else None."""
    p = state.raw_params["params"]
    at, rt = p["album_embed"]["embedding"], p["artist_embed"]["embedding"]
    tx = state.tx
    if getattr(tx, "lazy", False) and hasattr(tx, "_lazy_state") and at.is_cuda and at.shape[1] == rt.shape[1]:
        return at, rt
    return None


def _pack_group(xs, n, n_artists):
    """One int32 host buffer for a group of playlists: [next_offsets as int64 (K + 1) | ctx_album K n | ctx_artist K n |
    next_album | next_artist], and the int64 offsets.  Artist ids are range-checked (album ids are hashed: any int32)."""
    K = len(xs)
    nexts_a = [_host_ids(x["next_album"]) for x in xs]
    nexts_r = [_host_ids(x["next_artist"]) for x in xs]
    lens = np.array([a.size for a in nexts_a], dtype=np.int64)
    if (lens < 1).any() or any(a.size != r.size for a, r in zip(nexts_a, nexts_r)):
        raise ValueError("every playlist needs a non-empty next list with one artist per album (lengths %s)"
                         % [(a.size, r.size) for a, r in zip(nexts_a, nexts_r)])
    off = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    buf = np.empty(2 * (K + 1) + 2 * K * n + 2 * total, dtype=np.int32)
    buf[:2 * (K + 1)] = off.view(np.int32)
    p = 2 * (K + 1)
    buf[p:p + K * n] = np.concatenate([_host_ids(x["album_context"]) for x in xs])
    buf[p + K * n:p + 2 * K * n] = np.concatenate([_host_ids(x["artist_context"]) for x in xs])
    q = p + 2 * K * n
    buf[q:q + total] = np.concatenate(nexts_a)
    buf[q + total:q + 2 * total] = np.concatenate(nexts_r)
    art = np.concatenate([buf[p + K * n:q], buf[q + total:]])
    if art.min() < 0 or art.max() >= n_artists:
        raise IndexError("artist id out of range [0, %d)" % n_artists)
    return buf, off


def train_steps(state, train_it, num_steps, regularization, sampler, group=64):
    """The training loop of train_spotify.py:255-259 for `num_steps` playlists drawn from `train_it` (the reference's
    feature dicts, without negatives): per playlist what ``sampler.fill(x, step)`` + ``train_step(state, x, regularization)``
    compute, bit for bit, issued `group` playlists per library call -- one upload of the group's contexts and next lists,
    one launch that draws every step's negatives and assembles its id lists, then the steps' own launches
    (esr_spotify_train_steps).  The step number of a playlist is the lazy optimizer's step counter for that step, so a
    restored run continues the same negative stream.  Returns (state, losses): float32 [num_steps] on the tables' device.

    ValueError for mixed context lengths within a call or an empty next list, IndexError for an artist id outside the
    artist table.  A state that is not on train_step's one-call path (optimizer not lazy, tables of unequal width) runs
    the per-playlist loop."""
    if num_steps < 1 or group < 1:
        raise ValueError("num_steps and group must be >= 1, got %d and %d" % (num_steps, group))
    xs = [next(train_it) for _ in range(num_steps)]
    n = _context_length(xs)
    tables = _fused(state)
    if tables is None:
        losses = []
        for x in xs:
            lz = state.opt_state.get("_lazy") if isinstance(state.opt_state, dict) else None
            step = (lz["step"] if lz else int(state.step)) + 1
            state, loss = train_step(state, sampler.fill(dict(x), step), regularization)
            losses.append(loss)
        return state, torch.stack(losses).float()
    at, rt = tables
    dev, tx = at.device, state.tx
    lz = tx._lazy_state(state.raw_params, state.opt_state)
    tr = state.opt_state["trace"]["params"]
    last_a, last_r = lz["last"][("params", "album_embed", "embedding")], lz["last"][("params", "artist_embed", "embedding")]
    if sampler.n_artists > rt.shape[0]:
        raise IndexError("the sampler's corpus may name artists up to %d, the artist table has %d rows"
                         % (sampler.n_artists, rt.shape[0]))
    losses = torch.empty(num_steps, dtype=torch.float32, device=dev)
    for g0 in range(0, num_steps, group):
        chunk = xs[g0:g0 + group]
        K = len(chunk)
        buf, off = _pack_group(chunk, n, rt.shape[0])
        total = int(off[-1])
        d = torch.from_numpy(buf).to(dev, non_blocking=True)
        p = 2 * (K + 1)
        q = p + 2 * K * n
        ops.spotify_train_steps(at, tr["album_embed"]["embedding"], last_a, rt, tr["artist_embed"]["embedding"], last_r,
                                d[p:p + K * n].view(K, n), d[p + K * n:q].view(K, n), d[q:q + total], d[q + total:],
                                off, d[:p].view(torch.int64), sampler.albums, sampler.artists, sampler.seed, lz["step"] + 1,
                                sampler.num_negatives, regularization, tx.lr, tx.momentum, losses=losses[g0:g0 + K])
        lz["step"] += K
        lz["dirty"] = True
        state = state.replace(step=state.step + K)
    return state, losses

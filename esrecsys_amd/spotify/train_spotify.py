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

"""Spotify eval on one MI355X: the per-playlist loop (eval_step P times) against eval_batch (one call for P playlists),
measured in the same run, at the reference shapes (2 262 292 tracks, 100 000 hashed albums, 295 861 artists,
feature_size 32, 5 context tracks, top 500).  Prints one JSON line per P.

    python benchmarks/spotify_eval_bench.py [--P 1,64,256,1000] [--reps 2]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3  # f32 vector / matrix peak of the MI355X (spec)


def _kernel_times(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.esr_kernel_timing_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, total, mn, mx = line.split("\t")
        out[name] = {"calls": int(calls), "ms": round(float(total), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", default="1,64,256,1000")
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    from esrecsys_amd import TrainState, _lib, optim
    from esrecsys_amd.spotify.models import SpotifyModel
    from esrecsys_amd.spotify.train_spotify import eval_batch, eval_step
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    T, n, F, k = 2_262_292, 5, 32, 500
    all_tracks = np.arange(T, dtype=np.int32)
    all_albums = rng.integers(0, 734_684, T).astype(np.int32)
    all_artists = rng.integers(0, 295_861, T).astype(np.int32)
    model = SpotifyModel(feature_size=F, device=dev)
    state = TrainState.create(apply_fn=model.apply, params=model.init(1701), tx=optim.sgd(1e-3, 0.98))
    d_trk, d_alb, d_art = (torch.from_numpy(a).to(dev) for a in (all_tracks, all_albums, all_artists))
    lib = _lib.load()
    for P in (int(v) for v in args.P.split(",")):
        ys = []
        for _ in range(P):
            pick = rng.integers(0, T, n)
            nx = rng.integers(0, T, int(rng.integers(1, 251)))
            ys.append({"album_context": torch.from_numpy(all_albums[pick]).to(dev),
                       "artist_context": torch.from_numpy(all_artists[pick]).to(dev),
                       "next_track": torch.from_numpy(all_tracks[nx]).to(dev),
                       "next_artist": torch.from_numpy(all_artists[nx]).to(dev)})
        eval_step(state, ys[0], d_trk, d_alb, d_art)
        eval_batch(state, ys[:2], d_trk, d_alb, d_art)
        torch.cuda.synchronize()
        loop_s, batch_s = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            want = torch.stack([eval_step(state, y, d_trk, d_alb, d_art) for y in ys])
            torch.cuda.synchronize()
            loop_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            got = eval_batch(state, ys, d_trk, d_alb, d_art)
            torch.cuda.synchronize()
            batch_s.append(time.perf_counter() - t0)
        lib.esr_kernel_timing(1)
        eval_batch(state, ys, d_trk, d_alb, d_art)
        torch.cuda.synchronize()
        kt = _kernel_times(lib)
        lib.esr_kernel_timing(0)
        tl, tb = min(loop_s), min(batch_s)
        score_ms = kt.get("spotify_eval_score_kernel", {}).get("ms", float("nan"))
        flop = 2.0 * P * n * T * 2 * F
        print(json.dumps({
            "bench": "spotify_eval", "P": P, "T": T, "n": n, "F": F, "k": k,
            "loop_ms_per_playlist": round(tl * 1e3 / P, 4), "batch_ms_per_playlist": round(tb * 1e3 / P, 4),
            "batch_ms_total": round(tb * 1e3, 3), "speedup": round(tl / tb, 2),
            "scoring_tflops_call": round(flop / tb / 1e12, 2), "scoring_tflops_kernel": round(flop / (score_ms * 1e-3) / 1e12, 2),
            "peak_fraction_kernel": round(flop / (score_ms * 1e-3) / 1e12 / PEAK_TF, 4),
            "metrics_equal": bool(torch.equal(got, want)), "kernels": kt}), flush=True)


if __name__ == "__main__":
    main()

"""Spotify training loop on one MI355X at the reference shapes of benchmarks/spotify_step.py (5 context tracks, 5-40 next
tracks, 64 negatives, feature_size 32, 100 000 hashed albums + 295 861 artists, 2 262 292 tracks): the existing loop
(sample_negative with NumPy + train_step on host features, one playlist per iteration) against train_steps (negatives
drawn on the device, `group` playlists per library call) on the same playlists, in one session.  Prints one JSON line.

    python benchmarks/spotify_steps_bench.py [--steps 2048] [--group 64] [--reps 3]
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


def _kernel_times(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.esr_kernel_timing_read(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, total, mn, mx = line.split("\t")
        out[name] = {"calls": int(calls), "ms": float(total), "min_ms": float(mn), "max_ms": float(mx)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2048)
    ap.add_argument("--group", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from esrecsys_amd import TrainState, _lib, optim
    from esrecsys_amd.spotify.models import SpotifyModel
    from esrecsys_amd.spotify.train_spotify import NegativeSampler, sample_negative, train_step, train_steps
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    T, o = 2_262_292, 64
    all_tracks = np.arange(T, dtype=np.int32)
    all_albums = rng.integers(0, 734_684, T).astype(np.int32)
    all_artists = rng.integers(0, 295_861, T).astype(np.int32)
    model = SpotifyModel(feature_size=32, device=dev)

    def fresh():
        return TrainState.create(apply_fn=model.apply, params=model.init(1701), tx=optim.sgd(1e-3, 0.98))

    playlists = []
    for _ in range(64):
        m = int(rng.integers(5, 40))
        pick = rng.integers(0, T, 5 + m)
        playlists.append({"track_context": all_tracks[pick[:5]], "album_context": all_albums[pick[:5]],
                          "artist_context": all_artists[pick[:5]], "next_track": all_tracks[pick[5:]],
                          "next_album": all_albums[pick[5:]], "next_artist": all_artists[pick[5:]]})
    feed = lambda count: (dict(playlists[i % len(playlists)]) for i in range(count))  # noqa: E731
    sampler = NegativeSampler(all_tracks, all_albums, all_artists, o, 1701, model.num_artists, dev)
    K = args.steps

    def loop(state):
        nrng = np.random.default_rng(1)
        for x in feed(K):
            sample_negative(x, nrng, o, all_tracks, all_albums, all_artists)
            state, loss = train_step(state, x, 10.0)
        return state, loss

    state_l, state_g = fresh(), fresh()
    for x in feed(8):
        sample_negative(x, rng, o, all_tracks, all_albums, all_artists)
        state_l, _ = train_step(state_l, x, 10.0)
    state_g, _ = train_steps(state_g, feed(args.group), args.group, 10.0, sampler, group=args.group)
    torch.cuda.synchronize()
    loop_s, group_s = [], []
    for _ in range(args.reps):            # alternating, same session
        t0 = time.perf_counter()
        state_l, loss_l = loop(state_l)
        torch.cuda.synchronize()
        loop_s.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        state_g, losses_g = train_steps(state_g, feed(K), K, 10.0, sampler, group=args.group)
        torch.cuda.synchronize()
        group_s.append(time.perf_counter() - t0)
    lib = _lib.load()
    lib.esr_kernel_timing(1)
    state_g, _ = train_steps(state_g, feed(4 * args.group), 4 * args.group, 10.0, sampler, group=args.group)
    torch.cuda.synchronize()
    kt = _kernel_times(lib)
    lib.esr_kernel_timing(0)
    asm = kt.get("spotify_assemble_kernel", {})
    tl, tg = min(loop_s), min(group_s)
    print(json.dumps({
        "bench": "spotify_steps", "steps": K, "group": args.group, "reps": args.reps,
        "shapes": "5 context, 5-40 next, 64 negatives, F=32, 100000 album rows, 295861 artists, T=2262292; lazy sgd momentum",
        "loop_steps_per_s": round(K / tl, 1), "loop_ms_per_step": round(tl / K * 1e3, 5),
        "train_steps_steps_per_s": round(K / tg, 1), "train_steps_ms_per_step": round(tg / K * 1e3, 5),
        "speedup": round(tl / tg, 3), "loop_s_all": [round(v, 4) for v in loop_s], "train_steps_s_all": [round(v, 4) for v in group_s],
        "assemble_launch_calls": asm.get("calls"), "assemble_launch_ms_mean": (asm["ms"] / asm["calls"]) if asm else None,
        "assemble_launch_ms_min": asm.get("min_ms"), "assemble_launch_ms_max": asm.get("max_ms"),
        "loss_loop_last": float(loss_l), "loss_train_steps_last": float(losses_g[-1]),
        "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()

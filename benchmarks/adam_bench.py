"""Dense against lazy optax.adam (optim.adam(lazy=True)) on the reference's two models: one JSON line per leg with the
steps/s of each, warmed up and timed with HIP events around `--steps` steps.

    python benchmarks/adam_bench.py [--steps 50] [--warmup 10] [--legs stl_c2,glove_ref,glove_c3]

Legs: stl_c2 = Shop-The-Look triplet step, two 1 M x 128 towers, B = 8192 (uniform ids); glove_ref = GloVe at the reference's
defaults (V = 465 537, D = 64, B = 2048, Zipf ids); glove_c3 = GloVe V = 465 537, D = 256, B = 65 536 (Zipf ids)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _zipf(rng, V, n, a=1.1):
    return ((rng.zipf(a, n) - 1) % V).astype(np.int32)


def _time(step, state, batches, warmup, steps):
    for i in range(warmup):
        state = step(state, batches[i % len(batches)])
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        state = step(state, batches[(warmup + i) % len(batches)])
    t1.record()
    t1.synchronize()
    return steps / (t0.elapsed_time(t1) / 1e3), state


MODES = (("dense", False), ("lazy", True))


def _ratio(out):
    if "dense_steps_per_s" in out and "lazy_steps_per_s" in out:
        out["lazy_over_dense"] = out["lazy_steps_per_s"] / out["dense_steps_per_s"]
    return out


def glove_leg(name, V, D, B, warmup, steps, dev):
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.wikipedia.models import Glove
    from esrecsys_amd.wikipedia.train_cooccurence import apply_model, update_model
    rng = np.random.default_rng(0)
    nb = 16
    batches = [(torch.from_numpy(_zipf(rng, V, 2 * B).reshape(2, B)).to(dev),
                torch.from_numpy(rng.uniform(0.5, 300, B).astype(np.float32)).to(dev)) for _ in range(nb)]

    def step(state, b):
        grads, _ = apply_model(state, b[0], b[1])
        return update_model(state, grads)
    out = {"leg": name, "V": V, "D": D, "B": B, "steps": steps, "warmup": warmup}
    for key, lazy in MODES:
        model = Glove(num_embeddings=V, features=D, device=dev)
        state = TrainState.create(apply_fn=model.apply, params=model.init(1701, None)["params"], tx=optim.adam(1e-3, lazy=lazy))
        out[key + "_steps_per_s"], state = _time(step, state, batches, warmup, steps)
        del state, model
        torch.cuda.empty_cache()
    return _ratio(out)


def stl_leg(name, V, D, B, warmup, steps, dev):
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.pinterest.models import STLModel
    from esrecsys_amd.pinterest.train_shop_the_look import train_step
    rng = np.random.default_rng(0)
    nb = 16
    batches = [tuple(torch.from_numpy(rng.integers(0, V, B).astype(np.int32)).to(dev) for _ in range(3)) for _ in range(nb)]

    def step(state, b):
        return train_step(state, b[0], b[1], b[2], 0.1, B)[0]
    out = {"leg": name, "V": V, "D": D, "B": B, "steps": steps, "warmup": warmup}
    for key, lazy in MODES:
        stl = STLModel(output_size=D, num_scenes=V, num_products=V, device=dev)
        state = TrainState.create(apply_fn=stl.apply, params=stl.init(0, None, None, None), tx=optim.adam(1e-3, lazy=lazy))
        out[key + "_steps_per_s"], state = _time(step, state, batches, warmup, steps)
        del state, stl
        torch.cuda.empty_cache()
    return _ratio(out)


LEGS = {
    "stl_c2": lambda w, s, d: stl_leg("stl_triplet_c2", 1 << 20, 128, 8192, w, s, d),
    "glove_ref": lambda w, s, d: glove_leg("glove_reference_defaults", 465537, 64, 2048, w, s, d),
    "glove_c3": lambda w, s, d: glove_leg("glove_c3", 465537, 256, 65536, w, s, d),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--modes", default="dense,lazy", help="dense,lazy or one of them (to profile one mode)")
    a = ap.parse_args()
    global MODES
    MODES = tuple(m for m in MODES if m[0] in a.modes.split(","))
    dev = torch.device("cuda", 0)
    for leg in a.legs.split(","):
        print(json.dumps(LEGS[leg](a.warmup, a.steps, dev)), flush=True)


if __name__ == "__main__":
    main()

"""Row-sparse Adagrad against lazy Adam (optim.adam(lr, lazy=True)) on the row-sharded steps at world 1 THROUGH the exchange
machinery (ESR_SHARDED_WORLD1_DIRECT=0: bucket, self-exchange, owner-side gather or catch-up-and-serve, gradient rows,
owner-side update): one JSON line per leg with the steps/s of each, timed with HIP events around one
sharded_train_steps call of `--steps` steps after `--warmup` steps.

    python benchmarks/sharded_adam_bench.py [--steps 50] [--warmup 10] [--legs trip_c2,glove_ref,glove_b65536]

Legs: trip_c2 = Shop-The-Look triplet step, two 1 M x 128 towers, B = 8192 (uniform ids); glove_ref = GloVe at the
reference's defaults (V = 465 537, D = 64, B = 2048, Zipf ids); glove_b65536 = the same with B = 65 536."""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _zipf(rng, V, n, a=1.1):
    return ((rng.zipf(a, n) - 1) % V).astype(np.int32)


def _time(run, batches, warmup, steps):
    run([batches[i % len(batches)] for i in range(warmup)])
    torch.cuda.synchronize()
    timed = [batches[(warmup + i) % len(batches)] for i in range(steps)]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    run(timed)
    t1.record()
    t1.synchronize()
    return steps / (t0.elapsed_time(t1) / 1e3)


def _optimizers():
    from esrecsys_amd import optim
    return (("adagrad", 0.05), ("lazy_adam", optim.adam(1e-3, lazy=True)))


def _ratio(out):
    out["lazy_adam_over_adagrad"] = out["lazy_adam_steps_per_s"] / out["adagrad_steps_per_s"]
    return out


def trip_leg(name, V, D, B, warmup, steps, dev):
    from esrecsys_amd import ops, sharded
    rng = np.random.default_rng(0)
    batches = [tuple(torch.from_numpy(rng.integers(0, V, B).astype(np.int32)).to(dev) for _ in range(3)) for _ in range(16)]
    out = {"leg": name, "V": V, "D": D, "B": B, "steps": steps, "warmup": warmup}
    for key, lr in _optimizers():
        adam = not isinstance(lr, float)
        tabs = [sharded.RowShardedTable((torch.randn(V, D, device=dev) * 0.05), None if adam else
                                        torch.full((V, D), 0.1, device=dev), V) for _ in range(2)]
        towers = sharded.ShardedTableGroup(tabs, kernels=ops)
        out[key + "_steps_per_s"] = _time(lambda bs: sharded.sharded_train_steps(
            "triplet", (towers,), bs, regularization=0.1, global_batch_size=float(B), lr=lr), batches, warmup, steps)
        del towers, tabs
        torch.cuda.empty_cache()
    return _ratio(out)


def glove_leg(name, V, D, B, warmup, steps, dev):
    from esrecsys_amd import ops, sharded
    rng = np.random.default_rng(0)
    batches = [(torch.from_numpy(_zipf(rng, V, 2 * B).reshape(2, B)).to(dev),
                torch.from_numpy(rng.uniform(0.5, 300, B).astype(np.float32)).to(dev)) for _ in range(16)]
    out = {"leg": name, "V": V, "D": D, "B": B, "steps": steps, "warmup": warmup}
    for key, lr in _optimizers():
        adam = not isinstance(lr, float)
        groups = tuple(sharded.ShardedTableGroup([sharded.RowShardedTable(
            torch.randn(V, w, device=dev) * 0.05, None if adam else torch.full((V, w), 0.1, device=dev), V)], kernels=ops)
            for w in (D, 1))
        out[key + "_steps_per_s"] = _time(lambda bs: sharded.sharded_train_steps(
            "glove", groups, bs, lr=lr, mode=ops.GLOVE_REFERENCE), batches, warmup, steps)
        del groups
        torch.cuda.empty_cache()
    return _ratio(out)


LEGS = {
    "trip_c2": lambda w, s, d: trip_leg("sharded_w1_triplet_c2", 1 << 20, 128, 8192, w, s, d),
    "glove_ref": lambda w, s, d: glove_leg("sharded_w1_glove_reference_defaults", 465537, 64, 2048, w, s, d),
    "glove_b65536": lambda w, s, d: glove_leg("sharded_w1_glove_b65536", 465537, 64, 65536, w, s, d),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", default=",".join(LEGS))
    a = ap.parse_args()
    os.environ["ESR_SHARDED_WORLD1_DIRECT"] = "0"  # the exchange machinery, not the one-pass single-GPU steps
    import torch.distributed as dist
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        for leg in a.legs.split(","):
            print(json.dumps(LEGS[leg](a.warmup, a.steps, dev)), flush=True)
    finally:
        from esrecsys_amd import rccl
        rccl.reset()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

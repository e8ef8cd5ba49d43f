"""CPU: esr_adam_catchup_gather (the owner-side catch-up-and-serve of lazy Adam) rejects bad arguments with ESR_EINVAL
before it touches a device, and the row-sharded and replicated steps refuse what lazy Adam cannot step: dense adam, sgd,
bf16 tables, overlap, and mixing a plain learning rate (row-sparse Adagrad) with Adam on one set of tables."""
import ctypes
import os

import pytest
import torch

from conftest import free_port

EINVAL = -1
A = 0x10000   # a 16-byte aligned address that is never dereferenced: every failing call below fails validation first
M = A + 4     # 4-byte aligned, not 16


@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


def _gather(lib, nt=1, tables=A, mus=A, nus=A, lasts=A, offs=None, D=4, srt=A, perm=A, n=3, served=A, step=2,
            arrays=True):
    offs = offs if offs is not None else [0, 10, 25][:nt + 1]
    arr = lambda v: (ctypes.c_void_p * max(nt, 1))(*([v] * max(nt, 1))) if arrays else None  # noqa: E731
    ro = (ctypes.c_int64 * len(offs))(*offs)
    return lib.esr_adam_catchup_gather(arr(tables), arr(mus), arr(nus), arr(lasts), ro, nt, D, srt, perm, n, served,
                                       step, 1e-3, 0.9, 0.999, 1e-8, None)


def test_catchup_gather_rejects_bad_arguments(lib):
    assert _gather(lib, tables=None) == EINVAL
    assert b"esr_adam_catchup_gather" in lib.esr_last_error()
    assert _gather(lib, arrays=False) == EINVAL
    assert b"null pointer" in lib.esr_last_error()
    assert _gather(lib, lasts=None) == EINVAL
    assert _gather(lib, srt=None) == EINVAL
    assert _gather(lib, perm=None) == EINVAL                  # a served buffer needs the permutation
    assert _gather(lib, nt=0, offs=[0]) == EINVAL
    assert _gather(lib, nt=3, offs=[0, 1, 2, 3]) == EINVAL
    assert _gather(lib, D=0) == EINVAL
    assert _gather(lib, D=2048) == EINVAL                     # beyond four float4 chunks per lane
    assert b"not supported" in lib.esr_last_error()
    assert _gather(lib, D=257) == EINVAL                      # beyond four scalar chunks per lane
    assert _gather(lib, n=-1) == EINVAL
    assert _gather(lib, step=0) == EINVAL
    assert _gather(lib, offs=[1, 10]) == EINVAL
    assert b"row_offsets[0]" in lib.esr_last_error()
    assert _gather(lib, nt=2, offs=[0, 10, 10]) == EINVAL     # an empty table
    assert _gather(lib, offs=[0, 1 << 31]) == EINVAL
    assert b"2^31" in lib.esr_last_error()
    assert _gather(lib, served=M) == EINVAL                   # float4 rows: 16-byte aligned served rows
    assert b"misaligned" in lib.esr_last_error()
    assert _gather(lib, srt=A + 2) == EINVAL
    assert _gather(lib, perm=A + 2) == EINVAL
    assert _gather(lib, tables=M) == EINVAL
    assert _gather(lib, mus=M) == EINVAL
    assert _gather(lib, lasts=A + 2) == EINVAL
    # what passes validation and has nothing to do: returns before any device work
    assert _gather(lib, n=0) == 0
    assert _gather(lib, n=0, D=1, served=M) == 0              # scalar rows: 4-byte aligned served rows are fine
    assert _gather(lib, n=0, served=None, perm=None) == 0     # catch up only
    assert _gather(lib, n=0, nt=2, D=256) == 0


def test_ops_catchup_gather_wants_device_tensors():
    from esrecsys_amd import ops
    t = torch.zeros(8, 4)
    last = torch.zeros(8, dtype=torch.int32)
    ids = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="one or two"):
        ops.adam_catchup_gather([], [], [], [], [0], ids, ids, 1, 1e-3)
    with pytest.raises(TypeError, match="CUDA"):
        ops.adam_catchup_gather([t], [t], [t], [last], [0, 8], ids, ids, 1, 1e-3)


def _refusals_worker(rank, port):
    import torch.distributed as dist
    from esrecsys_amd import ops, optim, replicated, sharded
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=1)
    try:
        def group(dtype=torch.float32, accum=True):
            ts = [sharded.RowShardedTable(torch.zeros(V, 8, dtype=dtype), torch.full((V, 8), 0.1) if accum else None, V)
                  for V in (11, 13)]
            return sharded.ShardedTableGroup(ts, kernels=ops)

        lazy = optim.adam(1e-3, lazy=True)
        # optimizers that move rows no step reads: refused before anything is looked up
        for tx in (optim.adam(1e-3), optim.sgd(1e-3, 0.9)):
            for call in (lambda: sharded.sharded_triplet_step(group(), None, None, None, 0.0, 8, tx),
                         lambda: sharded.sharded_inbatch_step(group(), None, None, 0.0, 8, 1.0, tx),
                         lambda: sharded.sharded_glove_step(group(), group(), None, None, 0, tx),
                         lambda: sharded.sharded_train_steps("triplet", (group(),), [], lr=tx)):
                with pytest.raises(TypeError, match="lazy=True"):
                    call()
            rep = replicated.ReplicatedTables([torch.zeros(11, 8)], [torch.full((11, 8), 0.1)], kernels=ops)
            with pytest.raises(TypeError, match="lazy=True"):
                replicated.replicated_glove_step(rep, rep, None, None, 0, tx)
            with pytest.raises(TypeError, match="lazy=True"):
                replicated.replicated_triplet_step(rep, None, None, None, 0.0, 8, tx)
            with pytest.raises(TypeError, match="lazy=True"):
                replicated.replicated_inbatch_step(rep, None, None, 0.0, 8, 1.0, tx)
        # bf16 tables: the one-GPU message
        with pytest.raises(TypeError, match="fp32 .* tables only .*bf16 tables"):
            sharded.sharded_triplet_step(group(torch.bfloat16), None, None, None, 0.0, 8, lazy)
        rep16 = replicated.ReplicatedTables([torch.zeros(11, 8, dtype=torch.bfloat16)], [None], kernels=ops)
        with pytest.raises(TypeError, match="fp32 .* tables only .*bf16 tables"):
            replicated.replicated_triplet_step(rep16, None, None, None, 0.0, 8, lazy)
        # overlap: batch k + 1's early lookup would catch up rows batch k is about to step
        with pytest.raises(ValueError, match="overlap"):
            sharded.sharded_train_steps("triplet", (group(),), [], lr=lazy, overlap=True)
        sharded.sharded_train_steps("triplet", (group(),), [], lr=lazy)   # (no batches, no overlap: nothing to do)
        # one set of tables steps one optimizer
        g = group(accum=False)
        assert g.use_optimizer(lazy, "t") == "adam" and g.opt_state["count"] == 0
        assert [tuple(m.shape) for m in g.opt_state["mu"]] == [(11, 8), (13, 8)]
        assert g.use_optimizer(optim.adam(1e-3, lazy=True), "t") == "adam"   # same hyper-parameters: the same books
        with pytest.raises(ValueError, match="other hyper-parameters"):
            g.use_optimizer(optim.adam(2e-3, lazy=True), "t")
        with pytest.raises(ValueError, match="stepped optim.adam"):
            sharded.sharded_triplet_step(g, None, None, None, 0.0, 8, 0.05)
        g = group()
        assert g.use_optimizer(0.05, "t") == "adagrad" and g.opt_state is None and g.adam_state() is None
        with pytest.raises(ValueError, match="stepped row-sparse Adagrad"):
            sharded.sharded_triplet_step(g, None, None, None, 0.0, 8, lazy)
        with pytest.raises(ValueError, match="accumulators"):
            group(accum=False).use_optimizer(0.05, "t")
        rep = replicated.ReplicatedTables([torch.zeros(11, 8)], [None], kernels=ops)
        assert rep.use_optimizer(lazy, "t") == "adam"
        with pytest.raises(ValueError, match="stepped optim.adam"):
            replicated.replicated_triplet_step(rep, None, None, None, 0.0, 8, 0.05)
        # kernels without lazy Adam (the CPU doubles): an error, not a quiet fallback
        with pytest.raises(TypeError, match="no lazy Adam"):
            sharded.ShardedTableGroup([sharded.RowShardedTable(torch.zeros(5, 4), None, 5)],
                                      kernels=object()).use_optimizer(lazy, "t")
    finally:
        dist.destroy_process_group()


def test_sharded_and_replicated_refuse_what_lazy_adam_cannot_step():
    import torch.multiprocessing as mp
    mp.spawn(_refusals_worker, args=(free_port(),), nprocs=1, join=True)

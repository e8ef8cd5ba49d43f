"""CPU: the lazy Adam entry points (esr_adam_catchup_rows2, esr_sparse_adam_step_lazy, esr_adam_flush) reject bad
arguments with ESR_EINVAL before they touch a device, and the optimizer object refuses what it cannot step lazily."""
import ctypes
import os

import pytest
import torch

EINVAL = -1
A = 0x10000   # a 16-byte aligned address that is never dereferenced: every call below fails validation first
M = A + 4     # 4-byte aligned, not 16


@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


def _catchup(lib, table0=A, mu0=A, nu0=A, last0=A, V0=10, D0=4, ids0=A, n0=3, mod0=0,
             table1=None, mu1=None, nu1=None, last1=None, V1=0, D1=0, ids1=None, n1=0, mod1=0, step=2):
    return lib.esr_adam_catchup_rows2(table0, mu0, nu0, last0, V0, D0, ids0, n0, mod0, table1, mu1, nu1, last1, V1, D1,
                                      ids1, n1, mod1, step, 1e-3, 0.9, 0.999, 1e-8, None)


def test_catchup_rejects_bad_arguments(lib):
    assert _catchup(lib, table0=None) == EINVAL
    assert b"null pointer" in lib.esr_last_error()
    assert _catchup(lib, ids0=None) == EINVAL
    assert _catchup(lib, last0=None) == EINVAL
    assert _catchup(lib, D0=0) == EINVAL
    assert _catchup(lib, V0=0) == EINVAL
    assert _catchup(lib, V0=1 << 31) == EINVAL
    assert _catchup(lib, n0=-1) == EINVAL
    assert _catchup(lib, mod0=-2) == EINVAL
    assert _catchup(lib, step=0) == EINVAL
    assert _catchup(lib, D0=2048) == EINVAL                   # beyond four float4 chunks per lane
    assert b"not supported" in lib.esr_last_error()
    assert _catchup(lib, table0=M) == EINVAL                  # misaligned rows
    assert b"aligned" in lib.esr_last_error()
    assert _catchup(lib, nu0=M) == EINVAL
    assert _catchup(lib, last0=A + 2) == EINVAL
    # the optional second table is validated as strictly as the first
    assert _catchup(lib, table1=A, mu1=A, nu1=None, last1=A, V1=5, D1=1, ids1=A, n1=3) == EINVAL
    assert _catchup(lib, table1=A, mu1=A, nu1=A, last1=A, V1=0, D1=1, ids1=A, n1=3) == EINVAL
    assert _catchup(lib, table1=A, mu1=A, nu1=A, last1=A, V1=5, D1=0, ids1=A, n1=3) == EINVAL
    assert _catchup(lib, table1=M, mu1=A, nu1=A, last1=A, V1=5, D1=1, ids1=A, n1=3) == EINVAL


def _step(lib, ntables=1, D=4, n=5, step=3, ptr=A, offsets=(0, 10, 20), grad=A, vids=A, null_arrays=False):
    arr = (ctypes.c_void_p * 2)(ptr, ptr)
    offs = (ctypes.c_int64 * 3)(*offsets)
    if null_arrays:
        return lib.esr_sparse_adam_step_lazy(None, None, None, None, None, ntables, D, vids, A, n, grad, 1e-3, 0.9, 0.999,
                                             1e-8, step, None)
    return lib.esr_sparse_adam_step_lazy(arr, arr, arr, arr, offs, ntables, D, vids, A, n, grad, 1e-3, 0.9, 0.999, 1e-8,
                                         step, None)


def test_sparse_step_rejects_bad_arguments(lib):
    assert _step(lib, null_arrays=True) == EINVAL
    assert b"null pointer" in lib.esr_last_error()
    assert _step(lib, ptr=None) == EINVAL                     # a null table inside the arrays
    assert _step(lib, ntables=0) == EINVAL
    assert _step(lib, ntables=3) == EINVAL
    assert _step(lib, D=0) == EINVAL
    assert _step(lib, D=4096) == EINVAL
    assert _step(lib, n=-1) == EINVAL
    assert _step(lib, step=0) == EINVAL
    assert _step(lib, ptr=M) == EINVAL                        # misaligned table / mu / nu
    assert b"aligned" in lib.esr_last_error()
    assert _step(lib, grad=M) == EINVAL
    assert _step(lib, vids=A + 1) == EINVAL
    assert _step(lib, offsets=(0, 0, 0)) == EINVAL            # an empty table
    assert _step(lib, offsets=(5, 10, 20)) == EINVAL          # virtual rows start at 0
    assert _step(lib, ntables=2, offsets=(0, 1 << 30, (1 << 31) + 5)) == EINVAL


def test_flush_rejects_bad_arguments(lib):
    f = lambda **kw: lib.esr_adam_flush(kw.get("table", A), kw.get("mu", A), kw.get("nu", A), kw.get("last", A),  # noqa
                                        kw.get("V", 10), kw.get("D", 4), kw.get("step", 3), 1e-3, 0.9, 0.999, 1e-8, None)
    assert f(table=None) == EINVAL
    assert f(last=None) == EINVAL
    assert f(V=0) == EINVAL
    assert f(D=0) == EINVAL
    assert f(D=2048) == EINVAL
    assert f(step=-1) == EINVAL
    assert f(mu=M) == EINVAL
    assert f(last=A + 2) == EINVAL


def test_lazy_adam_is_an_option_of_adam():
    from esrecsys_amd import optim
    dense, lazy = optim.adam(1e-3), optim.adam(1e-3, lazy=True)
    assert dense.wants_dense and not getattr(dense, "needs_flush", False) and not dense.lazy
    assert not lazy.wants_dense and lazy.needs_flush and lazy.lazy
    # optax's state layout either way: {count, mu, nu}
    params = {"t": {"embedding": torch.zeros(8, 4)}}
    st = lazy.init(params)
    assert set(st) == {"count", "mu", "nu"} and st["count"] == 0
    assert set(lazy.to_optax_state(st)["0"]) == {"count", "mu", "nu"}


def test_lazy_adam_refuses_bf16_tables():
    from esrecsys_amd import optim
    with pytest.raises(TypeError, match="fp32"):
        optim.adam(1e-3, lazy=True).init({"t": {"embedding": torch.zeros(8, 4, dtype=torch.bfloat16)}})
    optim.adam(1e-3).init({"t": {"embedding": torch.zeros(8, 4, dtype=torch.bfloat16)}})  # (dense: unchanged)


def test_sharded_and_replicated_refuse_lazy_adam():
    from esrecsys_amd import optim, replicated, sharded
    tx = optim.adam(1e-3, lazy=True)
    with pytest.raises(TypeError, match="lazy"):
        sharded.sharded_triplet_step(None, None, None, None, 0.0, 8, tx)
    with pytest.raises(TypeError, match="lazy"):
        sharded.sharded_glove_step(None, None, None, None, 0, tx)
    with pytest.raises(TypeError, match="lazy"):
        sharded.sharded_inbatch_step(None, None, None, 0.0, 8, 1.0, tx)
    with pytest.raises(TypeError, match="lazy"):
        sharded.sharded_train_steps("triplet", (None,), [], lr=tx)
    with pytest.raises(TypeError, match="lazy"):
        replicated.replicated_glove_step(None, None, None, None, 0, tx)
    with pytest.raises(TypeError, match="lazy"):
        replicated.replicated_triplet_step(None, None, None, None, 0.0, 8, tx)
    with pytest.raises(TypeError, match="lazy"):
        replicated.replicated_inbatch_step(None, None, None, 0.0, 8, 1.0, tx)

"""CPU: the C ABI of esr_fpmc.hip -- the three symbols exported and bound, the geometry consistent with ``ops``, every refusal
arriving with the function's name before any launch (stand-in device pointers, never dereferenced), and the host refusals
of ``factorization.FPMC``, ``evaluate.split_last`` and the ``ops`` wrappers that need no device."""
import ctypes
import os

import numpy as np
import pytest

SYMBOLS = ["esr_fpmc_geometry", "esr_fpmc_sample", "esr_fpmc_fwd_bwd"]
EINVAL = -1
P = 256          # a stand-in device address: never dereferenced, the calls return before any launch
LIM = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


def refuses(lib, fn, call, msg, **kw):
    assert call(**kw) == EINVAL, kw
    err = lib.esr_last_error()
    assert err.startswith(fn + b":") and msg in err, (kw, err)


def test_symbols_are_exported_and_bound(lib):
    from esrecsys_amd import _lib, build
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), "libesr_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "esr_hip.h")).read()
    for name in SYMBOLS:
        assert "int %s(" % name in header
    assert "esr_fpmc.hip" in build.SOURCES and any(h.endswith("esr_fpmc_sample.h") for h in build.HEADERS)


def test_geometry(lib):
    from esrecsys_amd import ops
    window, rank, mult = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.esr_fpmc_geometry(ctypes.byref(window), ctypes.byref(rank), ctypes.byref(mult)) == 0
    assert (window.value, rank.value, mult.value) == ops.fpmc_geometry() == (8, 128, 4)
    for args in ((None, ctypes.byref(rank), ctypes.byref(mult)), (ctypes.byref(window), None, ctypes.byref(mult)),
                 (ctypes.byref(window), ctypes.byref(rank), None)):
        assert lib.esr_fpmc_geometry(*args) == EINVAL and lib.esr_last_error().startswith(b"esr_fpmc_geometry:")


def test_sample_arguments_are_rejected_without_a_device(lib):
    def sample(soff=8 * P, supos=P, sipos=2 * P, nnz_seq=30, roff=16 * P, ripos=3 * P, nnz_seen=25, nu=10, ni=20, window=3,
               seed=1, step0=0, K=2, B=64, u=4 * P, e=5 * P, c=6 * P, i=7 * P, j=9 * P, valid=10 * P, dropped=11 * P):
        return lib.esr_fpmc_sample(soff, supos, sipos, nnz_seq, roff, ripos, nnz_seen, nu, ni, window, seed, step0, K, B, u, e,
                                   c, i, j, valid, dropped, None)

    fn = b"esr_fpmc_sample"
    for name in ("soff", "supos", "sipos", "roff", "ripos", "u", "e", "c", "i", "j", "valid", "dropped"):
        refuses(lib, fn, sample, b"null pointer", **{name: None})
    for name in ("K", "B"):
        for bad in (0, -1, LIM + 1):
            refuses(lib, fn, sample, b"bad sizes K=", **{name: bad})
    for name in ("nnz_seq", "nnz_seen", "ni", "nu"):
        for bad in (0, -3, LIM + 1, 1 << 40):
            refuses(lib, fn, sample, b"bad sizes nu=", **{name: bad})
    refuses(lib, fn, sample, b"nu + 3 ni", nu=LIM - 59, ni=20)
    refuses(lib, fn, sample, b"nu + 3 ni", nu=1, ni=LIM // 3 + 1)
    assert sample(nu=LIM - 60, ni=20, soff=None) == EINVAL and b"null pointer" in lib.esr_last_error()     # 2^31 - 1 fits
    for window in (0, -1, 9, 64):
        refuses(lib, fn, sample, b"window=", window=window)
    refuses(lib, fn, sample, b"misaligned pointer", soff=8 * P + 4)
    refuses(lib, fn, sample, b"misaligned pointer", roff=16 * P + 4)
    refuses(lib, fn, sample, b"misaligned pointer", sipos=2 * P + 2)
    refuses(lib, fn, sample, b"misaligned pointer", c=6 * P + 1)
    refuses(lib, fn, sample, b"misaligned pointer", dropped=11 * P + 2)


def test_fwd_bwd_arguments_are_rejected_without_a_device(lib):
    def fwd(user=16 * P, nu=10, item=32 * P, nxt=48 * P, prev=64 * P, ni=20, D=8, sipos=P, nnz_seq=30, u=2 * P, e=3 * P, c=4 * P,
            i=5 * P, j=6 * P, valid=7 * P, B=64, ctx=8 * P, M=100, reg=0.01, loss=9 * P, diff=10 * P, grads=80 * P,
            ctx_ids=11 * P, failed=12 * P):
        return lib.esr_fpmc_fwd_bwd(user, nu, item, nxt, prev, ni, D, sipos, nnz_seq, u, e, c, i, j, valid, B, ctx, M, reg, loss,
                                    diff, grads, ctx_ids, failed, None)

    fn = b"esr_fpmc_fwd_bwd"
    for D in (0, -4, 1, 2, 6, 7, 30, 127, 129, 132, 256):
        refuses(lib, fn, fwd, b"D=", D=D)
    for name in ("user", "item", "nxt", "prev", "sipos", "u", "e", "c", "i", "j", "loss", "failed"):
        refuses(lib, fn, fwd, b"null pointer", **{name: None})
    refuses(lib, fn, fwd, b"null pointer (grads without", ctx=None)
    refuses(lib, fn, fwd, b"null pointer (grads without", ctx_ids=None)
    for name in ("nu", "ni", "nnz_seq", "B"):
        for bad in (0, -1, LIM + 1):
            refuses(lib, fn, fwd, b"bad sizes nu=", **{name: bad})
    refuses(lib, fn, fwd, b"nu + 3 ni", nu=LIM - 59, ni=20)
    for M in (-1, LIM + 1):
        refuses(lib, fn, fwd, b"bad sizes M=", M=M)
    for reg in (-0.01, float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, fwd, b"must be finite and not negative", reg=reg)
    for name, at in (("user", 16 * P + 4), ("item", 32 * P + 8), ("nxt", 48 * P + 4), ("prev", 64 * P + 8),
                     ("grads", 80 * P + 4), ("ctx", 8 * P + 4), ("u", 2 * P + 2), ("e", 3 * P + 1), ("c", 4 * P + 2),
                     ("valid", 7 * P + 1), ("ctx_ids", 11 * P + 2), ("sipos", P + 1)):
        refuses(lib, fn, fwd, b"misaligned pointer", **{name: at})


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import FPMC
    u, i = [0, 0, 1], [0, 1, 1]
    for window in (0, 9, -1):
        with pytest.raises(ValueError, match="window"):
            FPMC(u, i, window=window, rank=4)
    for rank in (0, 2, 6, 30, 132, 256, -4):
        with pytest.raises(ValueError, match="rank"):
            FPMC(u, i, rank=rank)
    with pytest.raises(ValueError, match="reg"):
        FPMC(u, i, rank=4, reg=-1.0)
    with pytest.raises(ValueError, match="optimizer"):
        FPMC(u, i, rank=4, optimizer="adam")
    with pytest.raises(ValueError, match="one length"):
        FPMC(u, [0, 1], rank=4)
    with pytest.raises(ValueError, match="at least one seen pair"):
        FPMC([], [], rank=4)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        FPMC(u, i, rank=4, device="cpu")


def test_split_last_on_the_host():
    from esrecsys_amd import evaluate
    ids = np.array([5, 6, 7, 1, 2, 9, 9, 9, 9, 3], np.int64)
    off = np.array([0, 3, 5, 5, 9, 10])
    ctx, co, truth, to, kept = evaluate.split_last(ids, off)
    assert ctx.tolist() == [5, 6, 9, 9, 9] and co.tolist() == [0, 2, 5] and truth.tolist() == [7, 9] and to.tolist() == [0, 1, 2]
    assert kept.tolist() == [0, 3] and ctx.dtype == truth.dtype and co.dtype == to.dtype
    ctx, co, truth, to, kept = evaluate.split_last(ids, off, n_last=2, min_length=2 + 1)
    assert ctx.tolist() == [5, 9, 9] and truth.tolist() == [6, 7, 9, 9] and kept.tolist() == [0, 3]
    for n_last, min_length in ((0, 3), (3, 3), (2, 1)):
        with pytest.raises(ValueError, match="n_last"):
            evaluate.split_last(ids, off, n_last=n_last, min_length=min_length)


def test_ops_refuse_host_tensors():
    import torch
    from esrecsys_amd import ops
    ids, off = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.fpmc_sample(off, ids, ids, off, ids, 1, 1, 1, 0, 0, 1, 4)
    t = torch.zeros(4, 4)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.fpmc_fwd_bwd(t, t, t, t, ids, ids, ids, ids, ids, ids, None, 0.0)

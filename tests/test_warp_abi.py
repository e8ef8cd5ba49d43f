"""CPU: the C ABI of esr_warp.hip -- the two symbols exported and bound, the geometry consistent with ``ops``, every refusal
arriving with the function's name before any launch (stand-in device pointers, never dereferenced), and the host refusals
of ``factorization.WARP`` and ``ops.warp_step`` that need no device."""
import ctypes
import os

import numpy as np
import pytest

SYMBOLS = ["esr_warp_geometry", "esr_warp_step"]
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
    from esrecsys_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), "libesr_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "esr_hip.h")).read()
    for name in SYMBOLS:
        assert "int %s(" % name in header


def test_geometry(lib):
    from esrecsys_amd import ops
    trials, rank, mult = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.esr_warp_geometry(ctypes.byref(trials), ctypes.byref(rank), ctypes.byref(mult)) == 0
    assert (trials.value, rank.value, mult.value) == ops.warp_geometry() == (255, 128, 4)
    assert ops.bpr_geometry() == (15, 128, 4)                                # BPR's own geometry is untouched
    for args in ((None, ctypes.byref(rank), ctypes.byref(mult)), (ctypes.byref(trials), None, ctypes.byref(mult)),
                 (ctypes.byref(trials), ctypes.byref(rank), None)):
        assert lib.esr_warp_geometry(*args) == EINVAL and lib.esr_last_error().startswith(b"esr_warp_geometry:")


def test_step_arguments_are_rejected_without_a_device(lib):
    def step(user=16 * P, nu=10, item=32 * P, ni=20, D=8, off=8 * P, upos=P, ipos=2 * P, nnz=30, weight=3 * P, seed=1, step=0,
             B=64, T=32, margin=1.0, reg=0.01, u=4 * P, i=5 * P, j=6 * P, valid=7 * P, trials=9 * P, loss=10 * P, diff=11 * P,
             grads=64 * P, failed=12 * P):
        return lib.esr_warp_step(user, nu, item, ni, D, off, upos, ipos, nnz, weight, seed, step, B, T, margin, reg, u, i, j,
                                 valid, trials, loss, diff, grads, failed, None)

    fn = b"esr_warp_step"
    for D in (0, -4, 1, 2, 6, 7, 30, 127, 129, 132, 256):
        refuses(lib, fn, step, b"D=", D=D)
    for name in ("nu", "ni", "nnz", "B"):
        for bad in (0, -1, LIM + 1, 1 << 40):
            refuses(lib, fn, step, b"bad sizes nu=", **{name: bad})
    for T in (0, -1, 256, 1 << 20):
        refuses(lib, fn, step, b"max_trials=", T=T)
    for margin in (float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, step, b"margin=", margin=margin)
    for reg in (-0.01, float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, step, b"must be finite and not negative", reg=reg)
    for name in ("user", "item", "off", "upos", "ipos", "weight", "u", "i", "j", "valid", "trials", "loss", "failed"):
        refuses(lib, fn, step, b"null pointer", **{name: None})
    refuses(lib, fn, step, b"misaligned pointer", user=16 * P + 4)
    refuses(lib, fn, step, b"misaligned pointer", item=32 * P + 8)
    refuses(lib, fn, step, b"misaligned pointer", grads=64 * P + 4)
    refuses(lib, fn, step, b"misaligned pointer", off=8 * P + 4)
    for name in ("upos", "ipos", "weight", "u", "i", "j", "valid", "trials", "loss", "diff", "failed"):
        refuses(lib, fn, step, b"misaligned pointer", **{name: 5 * P + 2})


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import WARP
    u, i = [0, 0, 1], [0, 1, 1]
    for rank in (0, 2, 6, 30, 132, 256, -4):
        with pytest.raises(ValueError, match="rank"):
            WARP(u, i, rank=rank)
    for reg in (-1.0, float("nan"), float("inf"), 1e60):
        with pytest.raises(ValueError, match="reg"):
            WARP(u, i, rank=4, reg=reg)
    for lr in (float("nan"), float("inf"), -float("inf"), 1e60):
        with pytest.raises(ValueError, match="lr"):
            WARP(u, i, rank=4, lr=lr)
    for margin in (float("nan"), float("inf"), -float("inf"), 1e60):
        with pytest.raises(ValueError, match="margin"):
            WARP(u, i, rank=4, margin=margin)
    for trials in (0, 256, -3):
        with pytest.raises(ValueError, match="max_trials"):
            WARP(u, i, rank=4, max_trials=trials)
    with pytest.raises(ValueError, match="rank_weight"):
        WARP(u, i, rank=4, rank_weight="linear")
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        WARP(u, i, rank=4, device="cpu")


def test_rank_weight_tables_and_their_refusals():
    from esrecsys_amd.factorization import warp_rank_weight
    h = warp_rank_weight("harmonic", 5)
    assert h.dtype == np.float32 and h.shape == (6,) and h[0] == 0 and h[1] == 1 and h[2] == 1.5
    assert h[5] == np.float32(1 + 1 / 2 + 1 / 3 + 1 / 4 + 1 / 5)
    big = warp_rank_weight("harmonic", 100000)                                # an fp64 cumulative sum rounded once
    assert big[-1] == np.float32(np.sum(1.0 / np.arange(1, 100001, dtype=np.float64)[::-1]))
    assert np.array_equal(warp_rank_weight("log1p", 3), np.log1p(np.arange(4.0)).astype(np.float32))
    own = [0.0, 2.0, 1.0]
    assert np.array_equal(warp_rank_weight(own, 2), np.array(own, np.float32))
    for bad in ([0.0, 1.0], [0.0, 1.0, 2.0, 3.0], [[0.0, 1.0, 2.0]]):
        with pytest.raises(ValueError, match="ni \\+ 1"):
            warp_rank_weight(bad, 2)
    for bad in ([0.0, -1.0, 1.0], [0.0, float("nan"), 1.0], [0.0, float("inf"), 1.0], [0.0, 1e60, 1.0]):
        with pytest.raises(ValueError, match="finite"):
            warp_rank_weight(bad, 2)
    with pytest.raises(ValueError, match="harmonic"):
        warp_rank_weight("linear", 2)


def test_ops_refuse_host_tensors():
    import torch
    from esrecsys_amd import ops
    ids = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.warp_step(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(5, dtype=torch.int64), ids, ids, torch.zeros(5), 0, 0, 4,
                      8, 1.0, 0.0)

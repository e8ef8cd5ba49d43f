"""CPU: the C ABI of esr_bpr.hip -- the three symbols exported and bound, the geometry consistent with ``ops``, every refusal
arriving with the function's name before any launch (stand-in device pointers, never dereferenced), and the host refusals
of ``factorization.BPR`` and the ``ops`` wrappers that need no device."""
import ctypes
import os

import pytest

SYMBOLS = ["esr_bpr_geometry", "esr_bpr_sample", "esr_bpr_fwd_bwd"]
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
    tries, rank, mult = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert lib.esr_bpr_geometry(ctypes.byref(tries), ctypes.byref(rank), ctypes.byref(mult)) == 0
    assert (tries.value, rank.value, mult.value) == ops.bpr_geometry() == (15, 128, 4)
    for args in ((None, ctypes.byref(rank), ctypes.byref(mult)), (ctypes.byref(tries), None, ctypes.byref(mult)),
                 (ctypes.byref(tries), ctypes.byref(rank), None)):
        assert lib.esr_bpr_geometry(*args) == EINVAL and lib.esr_last_error().startswith(b"esr_bpr_geometry:")


def test_sample_arguments_are_rejected_without_a_device(lib):
    def sample(off=8 * P, upos=P, ipos=2 * P, nu=10, ni=20, nnz=30, seed=1, step0=0, K=2, B=64, u=3 * P, i=4 * P, j=5 * P,
               valid=6 * P, dropped=7 * P):
        return lib.esr_bpr_sample(off, upos, ipos, nu, ni, nnz, seed, step0, K, B, u, i, j, valid, dropped, None)

    fn = b"esr_bpr_sample"
    for name in ("off", "upos", "ipos", "u", "i", "j", "valid", "dropped"):
        refuses(lib, fn, sample, b"null pointer", **{name: None})
    for name in ("K", "B"):
        for bad in (0, -1, LIM + 1):
            refuses(lib, fn, sample, b"bad sizes K=", **{name: bad})
    for name in ("nnz", "ni", "nu"):
        for bad in (0, -3, LIM + 1, 1 << 40):
            refuses(lib, fn, sample, b"bad sizes nu=", **{name: bad})
    refuses(lib, fn, sample, b"misaligned pointer", off=8 * P + 4)
    refuses(lib, fn, sample, b"misaligned pointer", ipos=2 * P + 2)
    refuses(lib, fn, sample, b"misaligned pointer", dropped=7 * P + 1)


def test_fwd_bwd_arguments_are_rejected_without_a_device(lib):
    def fwd(user=16 * P, nu=10, item=32 * P, ni=20, D=8, u=P, i=2 * P, j=3 * P, valid=4 * P, B=64, reg=0.01, loss=5 * P,
            diff=6 * P, grads=64 * P, failed=7 * P):
        return lib.esr_bpr_fwd_bwd(user, nu, item, ni, D, u, i, j, valid, B, reg, loss, diff, grads, failed, None)

    fn = b"esr_bpr_fwd_bwd"
    for D in (0, -4, 1, 2, 6, 7, 30, 127, 129, 132, 256):
        refuses(lib, fn, fwd, b"D=", D=D)
    for name in ("user", "item", "u", "i", "j", "loss", "failed"):
        refuses(lib, fn, fwd, b"null pointer", **{name: None})
    for name in ("nu", "ni", "B"):
        for bad in (0, -1, LIM + 1):
            refuses(lib, fn, fwd, b"bad sizes nu=", **{name: bad})
    for reg in (-0.01, float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, fwd, b"must be finite and not negative", reg=reg)
    refuses(lib, fn, fwd, b"misaligned pointer", user=16 * P + 4)
    refuses(lib, fn, fwd, b"misaligned pointer", item=32 * P + 8)
    refuses(lib, fn, fwd, b"misaligned pointer", grads=64 * P + 4)
    refuses(lib, fn, fwd, b"misaligned pointer", u=P + 2)
    refuses(lib, fn, fwd, b"misaligned pointer", valid=4 * P + 1)


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import BPR
    u, i = [0, 0, 1], [0, 1, 1]
    for rank in (0, 2, 6, 30, 132, 256, -4):
        with pytest.raises(ValueError, match="rank"):
            BPR(u, i, rank=rank)
    for reg in (-1.0, float("nan"), float("inf"), 1e60):
        with pytest.raises(ValueError, match="reg"):
            BPR(u, i, rank=4, reg=reg)
    for lr in (float("nan"), float("inf"), -float("inf"), 1e60):
        with pytest.raises(ValueError, match="lr"):
            BPR(u, i, rank=4, lr=lr)
    for batch in (0, -5, 2 ** 31):
        with pytest.raises(ValueError, match="batch"):
            BPR(u, i, rank=4, batch=batch)
    for opt in ("adam", "", None):
        with pytest.raises(ValueError, match="optimizer"):
            BPR(u, i, rank=4, optimizer=opt)
    with pytest.raises(ValueError, match="one length"):
        BPR(u, [0, 1], rank=4)
    with pytest.raises(TypeError, match="integer"):
        BPR([0.5, 1.0], [0, 1], rank=4)
    with pytest.raises(ValueError, match="at least one seen pair"):
        BPR([], [], rank=4)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        BPR(u, i, rank=4, device="cpu")


def test_ops_refuse_host_tensors():
    import torch
    from esrecsys_amd import ops
    ids = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.bpr_sample(torch.zeros(2, dtype=torch.int64), ids, ids, 1, 1, 0, 0, 1, 4)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.bpr_fwd_bwd(torch.zeros(4, 4), torch.zeros(4, 4), ids, ids, ids, None, 0.0)

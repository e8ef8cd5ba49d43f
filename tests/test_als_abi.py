"""CPU: the C ABI of esr_als.hip -- exported and bound, the size queries consistent with ``ops``, every refusal arriving with
the function's name before any launch (stand-in device pointers, never dereferenced; the row offsets are HOST memory and
real), and the host refusals of the module."""
import ctypes
import os

import numpy as np
import pytest

SYMBOLS = ["esr_als_max_rank", "esr_als_predict_max_rank", "esr_als_geometry", "esr_als_solve_workspace_bytes", "esr_als_solve_rows",
           "esr_als_predict"]
EINVAL, EWORKSPACE = -1, -3
P = 256   # a stand-in device address: never dereferenced, the calls return before any launch
OFFSETS = np.array([0, 3, 3, 10, 2000], np.int64)     # four rows; the last one is a long row


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
    assert fn in err and msg in err, (kw, err)


def test_symbols_are_exported_and_bound(lib):
    from esrecsys_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), "libesr_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_size_queries_agree_with_ops_and_the_module(lib):
    from esrecsys_amd import factorization, ops
    assert lib.esr_als_max_rank() == 64 == ops.als_max_rank() == factorization.max_rank()
    assert lib.esr_als_predict_max_rank() == 128 == ops.als_predict_max_rank() == factorization.predict_max_rank()
    assert ops.als_predict_max_rank() == ops.bpr_geometry()[1]               # every rank that trains can be served
    chunk, per_wg = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.esr_als_geometry(ctypes.byref(chunk), ctypes.byref(per_wg)) == 0
    assert (chunk.value, per_wg.value) == ops.als_geometry()
    assert chunk.value >= 2 and chunk.value % 2 == 0 and per_wg.value >= 1
    assert lib.esr_als_geometry(None, ctypes.byref(per_wg)) == EINVAL and b"esr_als_geometry" in lib.esr_last_error()
    ws = lib.esr_als_solve_workspace_bytes
    sizes = [ws(100, n, 32) for n in (0, 1, 1000, 100_000, 10_000_000)]
    assert sizes[0] > 0 and all(x <= y for x, y in zip(sizes, sizes[1:])), sizes
    assert ws(10, 10_000_000, 8) <= ws(10, 10_000_000, 64) and ws(10, 1000, 8) <= ws(1000, 1000, 8)
    assert ws(-3, -5, 0) == ws(0, 0, 1)
    # a row's partials: rank^2 + rank floats for every chunk of a long row
    long_len = chunk.value * per_wg.value + 1
    assert ws(1, long_len, 64) - ws(1, long_len - 1, 64) >= (per_wg.value + 1) * (64 * 64 + 64) * 4


def test_solve_arguments_are_rejected_without_a_device(lib):
    def solve(other=P, n_other=50, rank=8, off=OFFSETS.ctypes.data, cols=P, targets=P, a=0, b=4, reg=0.1, weighted=1,
              out=16 * P, failed=P, ws=P, ws_bytes=0):
        return lib.esr_als_solve_rows(other, n_other, rank, off, cols, targets, a, b, reg, weighted, out, failed, ws, ws_bytes,
                                      None)

    fn = b"esr_als_solve_rows"
    assert solve() == EWORKSPACE and fn in lib.esr_last_error()              # a good call gets as far as the workspace
    for rank in (0, -1, 65):
        refuses(lib, fn, solve, b"rank=", rank=rank)
    refuses(lib, fn, solve, b"bad size n_other", n_other=-1)
    refuses(lib, fn, solve, b"bad size n_other", n_other=1 << 31)
    refuses(lib, fn, solve, b"out of order", a=3, b=2)
    refuses(lib, fn, solve, b"out of order", a=-1)
    for reg in (0.0, -0.1, float("inf"), float("nan")):
        refuses(lib, fn, solve, b"must be finite and positive", reg=reg)
    refuses(lib, fn, solve, b"weighted=2", weighted=2)
    refuses(lib, fn, solve, b"null pointer", off=None)
    refuses(lib, fn, solve, b"null pointer", out=None)
    refuses(lib, fn, solve, b"null pointer", failed=None)
    refuses(lib, fn, solve, b"misaligned pointer", out=16 * P + 2)
    refuses(lib, fn, solve, b"misaligned pointer", failed=P + 1)
    refuses(lib, fn, solve, b"misaligned pointer", cols=P + 2)
    refuses(lib, fn, solve, b"misaligned pointer", off=OFFSETS.ctypes.data + 4)
    refuses(lib, fn, solve, b"aliases other_factors", out=P)
    refuses(lib, fn, solve, b"aliases other_factors", other=P, n_other=50, out=P + 8 * 4)       # inside the table read
    assert solve(a=2, b=2, cols=None, targets=None, ws=None) == 0                                # no row: nothing to do
    need = lib.esr_als_solve_workspace_bytes(4, 2000, 8)
    assert solve(ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.esr_last_error()
    assert solve(ws=P + 8, ws_bytes=1 << 40) == EWORKSPACE and b"misaligned" in lib.esr_last_error()
    assert solve(ws=None, ws_bytes=1 << 40) == EWORKSPACE
    # past the workspace the host offsets are read: still before any launch
    refuses(lib, fn, solve, b"null pointer (ratings", cols=None, ws_bytes=1 << 40)
    refuses(lib, fn, solve, b"null pointer (ratings", targets=None, ws_bytes=1 << 40)
    refuses(lib, fn, solve, b"null pointer (ratings", other=None, ws_bytes=1 << 40)
    refuses(lib, fn, solve, b"null pointer (ratings", n_other=0, ws_bytes=1 << 40)
    bad = np.array([0, 5, 3, 10, 12], np.int64)
    refuses(lib, fn, solve, b"not ascending", off=bad.ctypes.data, ws_bytes=1 << 40)
    bad = np.array([-1, 0, 3, 10, 12], np.int64)
    refuses(lib, fn, solve, b"not ascending", off=bad.ctypes.data, ws_bytes=1 << 40)


def test_predict_arguments_are_rejected_without_a_device(lib):
    def predict(uf=P, nu=5, vf=2 * P, ni=7, rank=8, pos=P, offset=P, targets=None, nq=3, out=P):
        return lib.esr_als_predict(uf, nu, vf, ni, rank, pos, pos, offset, targets, nq, out, None)

    fn = b"esr_als_predict"
    for rank in (0, 129):
        refuses(lib, fn, predict, b"rank=", rank=rank)
    assert predict(rank=128, nq=0) == 0                                      # the predict kernel's own cap: accepted
    for name in ("nu", "ni", "nq"):
        refuses(lib, fn, predict, b"bad sizes", **{name: -1})
    refuses(lib, fn, predict, b"bad sizes", nu=1 << 31)
    refuses(lib, fn, predict, b"null pointer", pos=None)
    refuses(lib, fn, predict, b"null pointer", out=None)
    refuses(lib, fn, predict, b"null pointer (factors)", uf=None)
    refuses(lib, fn, predict, b"null pointer (factors)", vf=None)
    refuses(lib, fn, predict, b"misaligned pointer", offset=P + 4)
    refuses(lib, fn, predict, b"misaligned pointer", out=P + 2)
    assert predict(nq=0, pos=None, out=None, uf=None, vf=None) == 0          # no query: nothing to do


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import CENTERS, FactorizationError, RatingsALS
    assert CENTERS == ("user", "global", "none") and issubclass(FactorizationError, RuntimeError)
    u, i, r = [0, 0, 1], [0, 1, 1], [3.0, 4.0, 2.5]
    for rank in (0, 65, -2):
        with pytest.raises(ValueError, match="rank"):
            RatingsALS(u, i, r, rank=rank)
    for reg in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="reg"):
            RatingsALS(u, i, r, rank=2, reg=reg)
    with pytest.raises(ValueError, match="center"):
        RatingsALS(u, i, r, rank=2, center="item")
    with pytest.raises(ValueError, match="max_rows_per_launch"):
        RatingsALS(u, i, r, rank=2, max_rows_per_launch=0)
    with pytest.raises(ValueError, match="one length"):
        RatingsALS(u, i, r[:2], rank=2)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        RatingsALS(u, i, r, rank=2, device="cpu")


def test_ops_refuse_host_tensors_and_device_offsets():
    import torch
    from esrecsys_amd import ops
    t = torch.zeros(4, 2)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.als_predict(t, t, torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.als_solve_rows(t, np.zeros(2, np.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(1), 0, 1, 0.1, True, t,
                           torch.zeros(1, dtype=torch.int32))

"""CPU: the C ABI of the implicit-feedback entry points of esr_als.hip -- exported and bound, the geometry and workspace
queries monotone and consistent with ``ops``, every refusal arriving with the function's name before any launch (stand-in
device pointers, never dereferenced; the row offsets are HOST memory and real), and the host refusals of the module."""
import ctypes
import os

import numpy as np
import pytest

SYMBOLS = ["esr_als_gram_geometry", "esr_als_gram_workspace_bytes", "esr_als_gram", "esr_als_solve_rows_implicit"]
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
    assert err.startswith(fn + b":") and msg in err, (kw, err)


def test_symbols_are_exported_and_bound(lib):
    from esrecsys_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), "libesr_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_geometry_and_workspace_queries(lib):
    from esrecsys_amd import ops
    seg = ctypes.c_int(0)
    assert lib.esr_als_gram_geometry(ctypes.byref(seg)) == 0
    assert seg.value == ops.als_gram_geometry() and seg.value >= 2 and seg.value % 2 == 0
    assert lib.esr_als_gram_geometry(None) == EINVAL and lib.esr_last_error().startswith(b"esr_als_gram_geometry:")
    ws = lib.esr_als_gram_workspace_bytes
    S = seg.value
    sizes = [ws(n, 32) for n in (0, 1, S, S + 1, 100 * S, 10_000_000)]
    assert sizes[0] > 0 and all(x <= y for x, y in zip(sizes, sizes[1:])), sizes
    assert ws(10 * S, 8) <= ws(10 * S, 64) and ws(-5, 0) == ws(0, 1)
    # a segment's partial: rank^2 floats
    assert ws(S + 1, 64) - ws(S, 64) >= 64 * 64 * 4 and ws(2 * S, 64) == ws(S + 1, 64)
    # the row solve shares the explicit path's workspace query
    assert lib.esr_als_solve_workspace_bytes(4, 2000, 8) > 0


def test_gram_arguments_are_rejected_without_a_device(lib):
    def gram(factors=P, n=1000, rank=8, out=1024 * P, ws=P, ws_bytes=0):
        return lib.esr_als_gram(factors, n, rank, out, ws, ws_bytes, None)

    fn = b"esr_als_gram"
    assert gram() == EWORKSPACE and lib.esr_last_error().startswith(fn + b":")     # a good call gets as far as the workspace
    for rank in (0, -1, 65):
        refuses(lib, fn, gram, b"rank=", rank=rank)
    refuses(lib, fn, gram, b"bad size n", n=-1)
    refuses(lib, fn, gram, b"bad size n", n=1 << 31)
    refuses(lib, fn, gram, b"null pointer", out=None)
    refuses(lib, fn, gram, b"null pointer", factors=None)
    refuses(lib, fn, gram, b"misaligned pointer", out=1024 * P + 2)
    refuses(lib, fn, gram, b"misaligned pointer", factors=P + 1)
    refuses(lib, fn, gram, b"aliases factors", out=P)
    refuses(lib, fn, gram, b"aliases factors", out=P + 8 * 4)                     # inside the table read
    need = lib.esr_als_gram_workspace_bytes(1000, 8)
    assert gram(ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.esr_last_error()
    assert gram(ws=P + 8, ws_bytes=1 << 40) == EWORKSPACE and b"misaligned" in lib.esr_last_error()
    assert gram(ws=None, ws_bytes=1 << 40) == EWORKSPACE


def test_solve_arguments_are_rejected_without_a_device(lib):
    def solve(other=P, n_other=50, rank=8, gram=8 * P, off=OFFSETS.ctypes.data, cols=P, weights=P, a=0, b=4, reg=0.1,
              weighted=1, out=16 * P, failed=P, ws=P, ws_bytes=0):
        return lib.esr_als_solve_rows_implicit(other, n_other, rank, gram, off, cols, weights, a, b, reg, weighted, out,
                                               failed, ws, ws_bytes, None)

    fn = b"esr_als_solve_rows_implicit"
    assert solve() == EWORKSPACE and lib.esr_last_error().startswith(fn + b":")   # a good call gets as far as the workspace
    for rank in (0, -1, 65):
        refuses(lib, fn, solve, b"rank=", rank=rank)
    refuses(lib, fn, solve, b"bad size n_other", n_other=-1)
    refuses(lib, fn, solve, b"out of order", a=3, b=2)
    refuses(lib, fn, solve, b"out of order", a=-1)
    for reg in (0.0, -0.1, float("inf"), float("nan")):
        refuses(lib, fn, solve, b"must be finite and positive", reg=reg)
    refuses(lib, fn, solve, b"weighted=2", weighted=2)
    refuses(lib, fn, solve, b"null pointer", off=None)
    refuses(lib, fn, solve, b"null pointer", out=None)
    refuses(lib, fn, solve, b"null pointer", failed=None)
    refuses(lib, fn, solve, b"null pointer", gram=None)
    refuses(lib, fn, solve, b"misaligned pointer", out=16 * P + 2)
    refuses(lib, fn, solve, b"misaligned pointer", weights=P + 2)
    refuses(lib, fn, solve, b"misaligned pointer", gram=8 * P + 2)
    refuses(lib, fn, solve, b"misaligned pointer", cols=P + 2)
    refuses(lib, fn, solve, b"aliases other_factors", out=P)
    refuses(lib, fn, solve, b"aliases other_factors", other=P, n_other=50, out=P + 8 * 4)      # inside the table read
    refuses(lib, fn, solve, b"aliases gram", gram=16 * P)
    refuses(lib, fn, solve, b"aliases gram", gram=16 * P - 8 * 4)                               # its tail on the first row
    assert solve(a=2, b=2, cols=None, weights=None, ws=None) == 0                               # no row: nothing to do
    need = lib.esr_als_solve_workspace_bytes(4, 2000, 8)
    assert solve(ws_bytes=need - 1) == EWORKSPACE and b"workspace" in lib.esr_last_error()
    assert solve(ws=P + 8, ws_bytes=1 << 40) == EWORKSPACE and b"misaligned" in lib.esr_last_error()
    assert solve(ws=None, ws_bytes=1 << 40) == EWORKSPACE
    # past the workspace the host offsets are read: still before any launch
    refuses(lib, fn, solve, b"null pointer (ratings", cols=None, ws_bytes=1 << 40)
    refuses(lib, fn, solve, b"null pointer (ratings", weights=None, ws_bytes=1 << 40)
    bad = np.array([0, 5, 3, 10, 12], np.int64)
    refuses(lib, fn, solve, b"not ascending", off=bad.ctypes.data, ws_bytes=1 << 40)


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import FAIL_BAD_WEIGHT, ImplicitALS
    assert FAIL_BAD_WEIGHT == 1 << 29
    u, i = [0, 0, 1], [0, 1, 1]
    for rank in (0, 65, -2):
        with pytest.raises(ValueError, match="rank"):
            ImplicitALS(u, i, rank=rank)
    for reg in (0.0, -1.0, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="reg"):
            ImplicitALS(u, i, rank=2, reg=reg)
    for alpha in (0.0, -40.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            ImplicitALS(u, i, rank=2, alpha=alpha)
    with pytest.raises(ValueError, match="max_rows_per_launch"):
        ImplicitALS(u, i, rank=2, max_rows_per_launch=0)
    with pytest.raises(ValueError, match="one length"):
        ImplicitALS(u, i, [1.0, 2.0], rank=2)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ImplicitALS(u, i, rank=2, device="cpu")


def test_ops_refuse_host_tensors_and_device_offsets():
    import torch
    from esrecsys_amd import ops
    t = torch.zeros(4, 2)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.als_gram(t)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.als_solve_rows_implicit(t, torch.zeros(2, 2), np.zeros(2, np.int64), torch.zeros(1, dtype=torch.int32),
                                    torch.zeros(1), 0, 1, 0.1, True, t, torch.zeros(1, dtype=torch.int32))

"""CPU: the C ABI of esr_bag.hip -- the three symbols exported, bound and in the header, the geometry consistent with
``ops``, every refusal arriving with the function's name before any launch (stand-in device pointers, never dereferenced),
and the host refusals of ``factorization.HybridBPR`` and the ``ops`` wrappers that need no device."""
import ctypes
import os

import pytest

SYMBOLS = ["esr_bag_geometry", "esr_bag_sum", "esr_bag_expand"]
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
    from esrecsys_amd import build
    assert "esr_bag.hip" in build.SOURCES and any(h.endswith("esr_bag_rule.h") for h in build.HEADERS)


def test_geometry(lib):
    from esrecsys_amd import ops
    rank, mult = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.esr_bag_geometry(ctypes.byref(rank), ctypes.byref(mult)) == 0
    assert (rank.value, mult.value) == ops.bag_geometry() == (128, 4) == ops.bpr_geometry()[1:]
    for args in ((None, ctypes.byref(mult)), (ctypes.byref(rank), None)):
        assert lib.esr_bag_geometry(*args) == EINVAL and lib.esr_last_error().startswith(b"esr_bag_geometry:")


def _shared_refusals(lib, fn, call, outputs):
    for D in (0, -4, 1, 2, 6, 7, 30, 127, 129, 132, 256):
        refuses(lib, fn, call, b"D=", D=D)
    for name in ("table", "off", "feat", "failed") + outputs:
        refuses(lib, fn, call, b"null pointer", **{name: None})
    for name in ("nf", "nnz", "n_bags"):
        for bad in (0, -1, LIM + 1, 1 << 40):
            refuses(lib, fn, call, b"bad sizes nf=", **{name: bad})
    for bad in (-1, LIM + 1):
        refuses(lib, fn, call, b"bad sizes nf=", n=bad)
    refuses(lib, fn, call, b"misaligned pointer", table=16 * P + 4)
    refuses(lib, fn, call, b"misaligned pointer", table=16 * P + 8)
    refuses(lib, fn, call, b"misaligned pointer", off=8 * P + 4)
    refuses(lib, fn, call, b"misaligned pointer", feat=P + 2)
    refuses(lib, fn, call, b"misaligned pointer", weight=2 * P + 1)
    refuses(lib, fn, call, b"misaligned pointer", rows=3 * P + 2)
    refuses(lib, fn, call, b"misaligned pointer", failed=7 * P + 1)
    refuses(lib, fn, call, b"without rows", rows=None, n=21, n_bags=20)
    # weight and rows may be null; n = 0 is a no-op that launches nothing
    assert call(n=0) == 0 and call(n=0, weight=None, rows=None) == 0


def test_sum_arguments_are_rejected_without_a_device(lib):
    def bag_sum(table=16 * P, nf=10, D=8, off=8 * P, feat=P, weight=2 * P, nnz=30, n_bags=20, rows=3 * P, n=64, out=32 * P,
                failed=7 * P):
        return lib.esr_bag_sum(table, nf, D, off, feat, weight, nnz, n_bags, rows, n, out, failed, None)

    fn = b"esr_bag_sum"
    _shared_refusals(lib, fn, bag_sum, ("out",))
    refuses(lib, fn, bag_sum, b"misaligned pointer", out=32 * P + 4)
    refuses(lib, fn, bag_sum, b"misaligned pointer", out=32 * P + 8)


def test_expand_arguments_are_rejected_without_a_device(lib):
    def expand(table=16 * P, nf=10, D=8, off=8 * P, feat=P, weight=2 * P, nnz=30, n_bags=20, rows=3 * P, grads=48 * P,
               valid=4 * P, oo=24 * P, n=64, M=100, reg=0.01, out_feat=5 * P, out_grads=64 * P, failed=7 * P):
        return lib.esr_bag_expand(table, nf, D, off, feat, weight, nnz, n_bags, rows, grads, valid, oo, n, M, reg, out_feat,
                                  out_grads, failed, None)

    fn = b"esr_bag_expand"
    _shared_refusals(lib, fn, expand, ("grads", "oo", "out_feat", "out_grads"))
    for bad in (-1, LIM + 1, 1 << 40):
        refuses(lib, fn, expand, b"bad sizes M=", M=bad)
    for reg in (-0.01, float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, expand, b"must be finite and not negative", reg=reg)
    refuses(lib, fn, expand, b"misaligned pointer", grads=48 * P + 4)
    refuses(lib, fn, expand, b"misaligned pointer", out_grads=64 * P + 8)
    refuses(lib, fn, expand, b"misaligned pointer", oo=24 * P + 4)
    refuses(lib, fn, expand, b"misaligned pointer", valid=4 * P + 2)
    refuses(lib, fn, expand, b"misaligned pointer", out_feat=5 * P + 1)
    assert expand(n=0, valid=None) == 0


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import BPR, HybridBPR
    assert issubclass(HybridBPR, BPR)
    u, i = [0, 0, 1], [5, 6, 6]
    tags = ([5, 6, 6], [100, 100, 101], None)
    with pytest.raises(ValueError, match="identity is off"):
        HybridBPR(u, i, identity=(False, True), rank=4)
    with pytest.raises(ValueError, match="identity is off"):
        HybridBPR(u, i, user_features=([0, 1], [7, 7], None), identity=(True, False), rank=4)
    with pytest.raises(ValueError, match="given twice"):
        HybridBPR(u, i, item_features=([5, 6, 5], [100, 100, 100], None), rank=4)
    with pytest.raises(ValueError, match="given twice"):
        HybridBPR(u, i, user_features=([1, 1], [3, 3], [1.0, 2.0]), rank=4)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e60):
        with pytest.raises(ValueError, match="not finite"):
            HybridBPR(u, i, item_features=([5, 6], [100, 100], [1.0, bad]), rank=4)
    with pytest.raises(ValueError, match="item_features: entity id 7 occurs in no"):
        HybridBPR(u, i, item_features=([5, 7], [100, 100], None), rank=4)
    with pytest.raises(ValueError, match="user_features: entity id 2 occurs in no"):
        HybridBPR(u, i, user_features=([2], [100], None), rank=4)
    with pytest.raises(ValueError, match="one length"):
        HybridBPR(u, i, item_features=([5, 6], [100], None), rank=4)
    with pytest.raises(ValueError, match="one length"):
        HybridBPR(u, i, item_features=([5, 6], [100, 100], [1.0]), rank=4)
    with pytest.raises(TypeError, match="integer"):
        HybridBPR(u, i, item_features=([5.0, 6.0], [100, 100], None), rank=4)
    with pytest.raises(ValueError, match="entity_id, feature_id, weight"):
        HybridBPR(u, i, item_features=([5, 6], [100, 100]), rank=4)
    # BPR's own refusals still arrive
    for rank in (0, 2, 6, 132):
        with pytest.raises(ValueError, match="rank"):
            HybridBPR(u, i, item_features=tags, rank=rank)
    with pytest.raises(ValueError, match="reg"):
        HybridBPR(u, i, item_features=tags, rank=4, reg=-1.0)
    with pytest.raises(ValueError, match="optimizer"):
        HybridBPR(u, i, item_features=tags, rank=4, optimizer="adam")
    with pytest.raises(ValueError, match="at least one seen pair"):
        HybridBPR([], [], rank=4)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        HybridBPR(u, i, item_features=tags, rank=4, device="cpu")


def test_the_host_bag_table_puts_the_identity_row_first():
    import numpy as np
    from esrecsys_amd.factorization import _bag_table
    epos, fpos = np.array([2, 0, 2], np.int64), np.array([1, 0, 0], np.int64)
    off, feat, w = _bag_table(epos, fpos, np.array([0.5, 2.0, 4.0], np.float32), 3, True, "item")
    assert off.tolist() == [0, 2, 3, 6] and feat.tolist() == [0, 3, 1, 2, 3, 4] and w.tolist() == [1, 2, 1, 1, 4, 0.5]
    off, feat, w = _bag_table(epos, fpos, None, 3, False, "item")
    assert off.tolist() == [0, 1, 1, 3] and feat.tolist() == [0, 0, 1] and w is None
    off, feat, w = _bag_table(np.zeros(0, np.int64), np.zeros(0, np.int64), None, 3, True, "user")
    assert off.tolist() == [0, 1, 2, 3] and feat.tolist() == [0, 1, 2] and w is None


def test_ops_refuse_host_tensors():
    import torch
    from esrecsys_amd import ops
    ids, off = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.bag_sum(torch.zeros(4, 4), off, ids, None)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.bag_expand(torch.zeros(4, 4), off, ids, None, None, torch.zeros(1, 4), None, off, 3, 0.0)

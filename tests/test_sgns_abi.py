"""CPU: the C ABI of esr_sgns.hip -- the three symbols exported and bound, the geometry consistent with ``ops``, every refusal
arriving with the function's name before any launch (stand-in device pointers, never dereferenced), and the host refusals
of ``factorization.SGNS`` and the ``ops`` wrappers that need no device."""
import ctypes
import os

import pytest

SYMBOLS = ["esr_sgns_geometry", "esr_sgns_sample", "esr_sgns_fwd_bwd"]
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
    assert "esr_sgns.hip" in build.SOURCES and any(h.endswith("esr_sgns_sample.h") for h in build.HEADERS)


def test_geometry(lib):
    from esrecsys_amd import ops
    out = [ctypes.c_int(0) for _ in range(4)]
    assert lib.esr_sgns_geometry(*[ctypes.byref(v) for v in out]) == 0
    assert tuple(v.value for v in out) == ops.sgns_geometry() == (32, 16, 128, 4)
    for hole in range(4):
        args = [None if n == hole else ctypes.byref(v) for n, v in enumerate(out)]
        assert lib.esr_sgns_geometry(*args) == EINVAL and lib.esr_last_error().startswith(b"esr_sgns_geometry:")


def test_sample_arguments_are_rejected_without_a_device(lib):
    def sample(soff=8 * P, supos=P, sipos=2 * P, nnz_seq=30, nd=10, ni=20, window=3, negatives=5, keep=3 * P, alias=4 * P,
               seed=1, step0=0, K=2, B=64, c=5 * P, e=6 * P, o=7 * P, valid=9 * P, neg=10 * P, dropped=11 * P):
        return lib.esr_sgns_sample(soff, supos, sipos, nnz_seq, nd, ni, window, negatives, keep, alias, seed, step0, K, B, c, e,
                                   o, valid, neg, dropped, None)

    fn = b"esr_sgns_sample"
    for name in ("soff", "supos", "sipos", "keep", "alias", "c", "e", "o", "valid", "neg", "dropped"):
        refuses(lib, fn, sample, b"null pointer", **{name: None})
    for name in ("K", "B"):
        for bad in (0, -1, LIM + 1):
            refuses(lib, fn, sample, b"bad sizes K=", **{name: bad})
    for name in ("nnz_seq", "ni", "nd"):
        for bad in (0, -3, LIM + 1, 1 << 40):
            refuses(lib, fn, sample, b"bad sizes nd=", **{name: bad})
    refuses(lib, fn, sample, b"2 ni", ni=LIM // 2 + 1)
    assert sample(ni=LIM // 2, soff=None) == EINVAL and b"null pointer" in lib.esr_last_error()      # 2^31 - 2 rows fit
    for window in (0, -1, 33, 64):
        refuses(lib, fn, sample, b"window=", window=window)
    for negatives in (0, -1, 17, 64):
        refuses(lib, fn, sample, b"negatives=", negatives=negatives)
    for name, at in (("soff", 8 * P + 4), ("sipos", 2 * P + 2), ("supos", P + 1), ("keep", 3 * P + 2), ("alias", 4 * P + 1),
                     ("c", 5 * P + 1), ("neg", 10 * P + 2), ("dropped", 11 * P + 2)):
        refuses(lib, fn, sample, b"misaligned pointer", **{name: at})


def test_fwd_bwd_arguments_are_rejected_without_a_device(lib):
    def fwd(inn=16 * P, out=32 * P, ni=20, D=8, c=P, o=2 * P, neg=3 * P, valid=4 * P, B=64, negatives=5, reg=0.01, loss=5 * P,
            diff=6 * P, grads=48 * P, failed=7 * P):
        return lib.esr_sgns_fwd_bwd(inn, out, ni, D, c, o, neg, valid, B, negatives, reg, loss, diff, grads, failed, None)

    fn = b"esr_sgns_fwd_bwd"
    for D in (0, -4, 1, 2, 6, 7, 30, 127, 129, 132, 256):
        refuses(lib, fn, fwd, b"D=", D=D)
    for name in ("inn", "out", "c", "o", "neg", "loss", "failed"):
        refuses(lib, fn, fwd, b"null pointer", **{name: None})
    for name in ("ni", "B"):
        for bad in (0, -1, LIM + 1):
            refuses(lib, fn, fwd, b"bad sizes ni=", **{name: bad})
    refuses(lib, fn, fwd, b"2 ni", ni=LIM // 2 + 1)
    for negatives in (0, -1, 17):
        refuses(lib, fn, fwd, b"negatives=", negatives=negatives)
    refuses(lib, fn, fwd, b"gradient rows", B=LIM // 7 + 1, negatives=5)
    for reg in (-0.01, float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, fwd, b"must be finite and not negative", reg=reg)
    for name, at in (("inn", 16 * P + 4), ("out", 32 * P + 8), ("grads", 48 * P + 4), ("c", P + 2), ("o", 2 * P + 1),
                     ("neg", 3 * P + 2), ("valid", 4 * P + 1), ("loss", 5 * P + 2), ("diff", 6 * P + 1), ("failed", 7 * P + 2)):
        refuses(lib, fn, fwd, b"misaligned pointer", **{name: at})
    # valid, diff and grads may be null: the call gets past its checks only with a device, so only their checks are pinned
    refuses(lib, fn, fwd, b"null pointer", valid=None, diff=None, grads=None, inn=None)


def test_module_refuses_bad_arguments_on_the_host():
    from esrecsys_amd.factorization import SGNS
    d, i = [0, 0, 1], [0, 1, 1]
    for window in (0, 33, -1):
        with pytest.raises(ValueError, match="window"):
            SGNS(d, i, window=window, rank=4)
    for negatives in (0, 17, -1):
        with pytest.raises(ValueError, match="negatives"):
            SGNS(d, i, negatives=negatives, rank=4)
    for power in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="power"):
            SGNS(d, i, power=power, rank=4)
    for rank in (0, 2, 6, 30, 132, 256, -4):
        with pytest.raises(ValueError, match="rank"):
            SGNS(d, i, rank=rank)
    with pytest.raises(ValueError, match="reg"):
        SGNS(d, i, rank=4, reg=-1.0)
    with pytest.raises(ValueError, match="optimizer"):
        SGNS(d, i, rank=4, optimizer="adam")
    with pytest.raises(ValueError, match="one length"):
        SGNS(d, [0, 1], rank=4)
    with pytest.raises(ValueError, match="one length"):
        SGNS(d, i, time=[1.0, 2.0], rank=4, device="cpu")
    with pytest.raises(ValueError, match="gradient rows"):
        SGNS(d, i, rank=4, negatives=16, batch=2 ** 31 // 18 + 1, device="cpu")
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        SGNS(d, i, rank=4, device="cpu")


def test_ops_refuse_host_tensors():
    import torch
    from esrecsys_amd import ops
    ids, off = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.sgns_sample(off, ids, ids, 1, 1, 1, 1, ids[:1], ids[:1], 0, 0, 1, 4)
    t = torch.zeros(4, 4)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.sgns_fwd_bwd(t, t, ids, ids, ids.reshape(3, 1), None, 0.0)

"""CPU: the C ABI of esr_rerank.hip -- the three symbols exported, bound and in the header, the geometry consistent with the
restatement, every refusal arriving with the function's name before any launch (stand-in device pointers, never
dereferenced), and the host refusals of ``ops``, ``rerank`` and ``diversify`` that need no device."""
import ctypes
import os

import pytest

import _rerank_ref as rref

SYMBOLS = ["esr_rerank_geometry", "esr_rerank_mmr", "esr_rerank_ils"]
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
    header = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "include", "esr_hip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), "libesr_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert "int %s(" % name in header
    from esrecsys_amd import build
    assert "esr_rerank.hip" in build.SOURCES and any(h.endswith("esr_rerank_rule.h") for h in build.HEADERS)


def test_geometry(lib):
    from esrecsys_amd import ops
    g = ops.rerank_geometry(64, 500)
    assert (g["max_rank"], g["rank_multiple"], g["max_width"], g["max_cutoffs"]) == (128, 4, rref.MAX_WIDTH, 8)
    assert g["stage_bytes"] == rref.STAGE_BYTES and g["grid_cap"] >= 1 and (g["max_rank"], g["rank_multiple"]) == ops.bag_geometry()
    for D, width in ((4, 1), (4, 1024), (32, 1024), (36, 1024), (64, 512), (64, 513), (128, 256), (128, 257), (100, 327), (100, 328)):
        g = ops.rerank_geometry(D, width)
        assert bool(g["staged"]) == rref.staged(width, D), (D, width)
        assert g["lds_bytes"] == 16 * width + (4 * width * D if g["staged"] else 0)
        assert g["lds_bytes"] + 1024 <= 160 * 1024               # a CU's LDS, with room for the static exchange words
    outs = [ctypes.c_int(0) for _ in range(8)]

    def geometry(D=64, width=100, null=None):
        ptrs = [None if i == null else ctypes.byref(o) for i, o in enumerate(outs)]
        return lib.esr_rerank_geometry(D, width, *ptrs)

    assert geometry() == 0
    for i in range(8):
        refuses(lib, b"esr_rerank_geometry", geometry, b"null pointer", null=i)
    for D in (0, 2, 6, 129, 132):
        refuses(lib, b"esr_rerank_geometry", geometry, b"D=", D=D)
    for width in (0, -1, 1025):
        refuses(lib, b"esr_rerank_geometry", geometry, b"width=", width=width)


def _shared_refusals(lib, fn, call, outputs):
    for D in (0, -4, 1, 2, 6, 7, 30, 127, 129, 132, 256):
        refuses(lib, fn, call, b"D=", D=D)
    for width in (0, -1, 1025, 1 << 20):
        refuses(lib, fn, call, b"width=", width=width)
    for bad in (0, -1, LIM + 1, 1 << 40):
        refuses(lib, fn, call, b"bad sizes ni=", ni=bad)
    for bad in (-1, LIM + 1):
        refuses(lib, fn, call, b"bad sizes ni=", nq=bad)
    for name in ("rows", "cand", "failed") + outputs:
        refuses(lib, fn, call, b"null pointer", **{name: None})
    refuses(lib, fn, call, b"misaligned pointer", rows=16 * P + 4)
    refuses(lib, fn, call, b"misaligned pointer", rows=16 * P + 8)
    refuses(lib, fn, call, b"misaligned pointer", cand=P + 2)
    refuses(lib, fn, call, b"misaligned pointer", lengths=3 * P + 1)
    refuses(lib, fn, call, b"misaligned pointer", failed=7 * P + 2)
    for name in outputs:
        refuses(lib, fn, call, b"misaligned pointer", **{name: 9 * P + 2})
    # lengths may be null; nq = 0 is a no-op that launches nothing
    assert call(nq=0) == 0 and call(nq=0, lengths=None) == 0


def test_mmr_arguments_are_rejected_without_a_device(lib):
    def mmr(rows=16 * P, ni=10, D=8, cand=P, rel=2 * P, lengths=3 * P, nq=4, width=20, n_out=5, lam=0.5, out_pos=4 * P,
            out_item=5 * P, out_rel=6 * P, out_value=8 * P, out_length=9 * P, failed=7 * P):
        return lib.esr_rerank_mmr(rows, ni, D, cand, rel, lengths, nq, width, n_out, lam, out_pos, out_item, out_rel, out_value,
                                  out_length, failed, None)

    fn = b"esr_rerank_mmr"
    _shared_refusals(lib, fn, mmr, ("rel", "out_pos", "out_item", "out_rel", "out_value", "out_length"))
    for n_out in (0, -1, 21, 1025):
        refuses(lib, fn, mmr, b"n_out=", n_out=n_out)
    assert mmr(nq=0, n_out=20) == 0 and mmr(nq=0, n_out=1, width=1) == 0
    for lam in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        refuses(lib, fn, mmr, b"lam=", lam=lam)
    assert mmr(nq=0, lam=0.0) == 0 and mmr(nq=0, lam=1.0) == 0


def test_ils_arguments_are_rejected_without_a_device(lib):
    def ils(rows=16 * P, ni=10, D=8, cand=P, lengths=3 * P, nq=4, width=20, ks=(10, 100), nk=None, out=4 * P, valid=5 * P,
            failed=7 * P):
        arr = None if ks is None else (ctypes.c_int32 * max(1, len(ks)))(*ks)
        return lib.esr_rerank_ils(rows, ni, D, cand, lengths, nq, width, arr, len(ks or ()) if nk is None else nk, out, valid,
                                  failed, None)

    fn = b"esr_rerank_ils"
    _shared_refusals(lib, fn, ils, ("out", "valid"))
    refuses(lib, fn, ils, b"cutoffs", ks=None, nk=2)
    refuses(lib, fn, ils, b"cutoffs", ks=(), nk=0)
    refuses(lib, fn, ils, b"cutoffs", ks=tuple(range(1, 10)))
    for ks in ((0,), (-1, 5), (5, 5), (10, 3), (1, 2, 2)):
        refuses(lib, fn, ils, b"strictly ascending", ks=ks)
    assert ils(nq=0, ks=tuple(range(1, 9))) == 0 and ils(nq=0, ks=(5000,)) == 0


def test_ops_and_rerank_refuse_on_the_host():
    import torch
    from esrecsys_amd import ops, rerank
    rows, cand, rel = torch.zeros(4, 4), torch.zeros((2, 3), dtype=torch.int32), torch.zeros(2, 3)
    with pytest.raises(TypeError, match="no CPU fallback exists"):
        ops.rerank_mmr(rows, cand, rel, None, 0.5, 2)
    with pytest.raises(TypeError, match="no CPU fallback exists"):
        ops.rerank_ils(rows, cand, None, (2,))
    with pytest.raises(TypeError, match="no CPU fallback exists"):
        rerank.mmr(cand, rel, None, rows)
    with pytest.raises(TypeError, match="no CPU fallback exists"):
        rerank.intra_list_similarity(cand, None, rows, ks=(2,))
    for ks in ((), (0,), (3, 3), (5, 2), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            rerank.intra_list_similarity(cand, None, rows, ks=ks)
        with pytest.raises(ValueError):
            rerank.coverage(cand, None, ks)
    with pytest.raises(TypeError, match="sequence of ints"):
        rerank.intra_list_similarity(cand, None, rows, ks=3)


def test_shapes_are_refused_before_any_call():
    """the wrappers' own checks, on meta-free stand-ins: a tensor that claims to be on the device but is never read"""
    import torch
    from esrecsys_amd import ops

    class Fake(torch.Tensor):
        is_cuda = True

    def fake(t):
        return t.as_subclass(Fake)

    rows, cand, rel = fake(torch.zeros(4, 8)), fake(torch.zeros((2, 3), dtype=torch.int32)), fake(torch.zeros(2, 3))
    with pytest.raises(ValueError, match="rank = 6"):
        ops.rerank_mmr(fake(torch.zeros(4, 6)), cand, rel, None, 0.5, 2)
    with pytest.raises(ValueError, match=r"rows must be \[ni, rank\]"):
        ops.rerank_mmr(fake(torch.zeros(32)), cand, rel, None, 0.5, 2)
    with pytest.raises(ValueError, match="width = 1025"):
        ops.rerank_ils(rows, fake(torch.zeros((1, 1025), dtype=torch.int32)), None, (2,))
    with pytest.raises(ValueError, match="rel must have cand's shape"):
        ops.rerank_mmr(rows, cand, fake(torch.zeros(2, 4)), None, 0.5, 2)
    with pytest.raises(ValueError, match="one entry per query"):
        ops.rerank_mmr(rows, cand, rel, fake(torch.zeros(3, dtype=torch.int32)), 0.5, 2)
    for n_out in (0, 4):
        with pytest.raises(ValueError, match="n_out"):
            ops.rerank_mmr(rows, cand, rel, None, 0.5, n_out)
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            ops.rerank_mmr(rows, cand, rel, None, lam, 2)
    with pytest.raises(TypeError, match="must be torch.int32"):
        ops.rerank_mmr(rows, fake(torch.zeros((2, 3), dtype=torch.int64)), rel, None, 0.5, 2)
    with pytest.raises(ValueError, match="strictly ascending"):
        ops.rerank_ils(rows, cand, None, (4, 2))


def test_rerror_names_the_bit_and_mean_is_a_host_fp64_mean():
    import numpy as np
    import torch
    from esrecsys_amd import rerank
    with pytest.raises(rerank.RerankError, match="bit 30"):
        rerank._raise_failed(1 << 30, "mmr")
    with pytest.raises(rerank.RerankError, match="bit 29"):
        rerank._raise_failed(1 << 29, "mmr")
    rerank._raise_failed(0, "mmr")
    r = rerank.IntraListSimilarity((2, 4), torch.tensor([[0.5, 1.0], [0.25, 0.0], [9.0, 9.0]]),
                                   torch.tensor([[1, 1], [1, 0], [0, 0]], dtype=torch.int32))
    m = r.mean()
    assert m["ils"].dtype == np.float64 and m["ils"].tolist() == [0.375, 1.0] and m["n_valid"].tolist() == [2, 1]
    empty = rerank.IntraListSimilarity((2,), torch.zeros((0, 1)), torch.zeros((0, 1), dtype=torch.int32)).mean()
    assert empty["ils"].tolist() == [0.0] and empty["n_valid"].tolist() == [0]
    assert rerank.unit_rows(torch.tensor([[3.0, 4.0], [0.0, 0.0]])).tolist() == [[np.float32(0.6), np.float32(0.8)], [0, 0]]
    assert rerank.coverage(torch.tensor([[1, 2, 3], [2, 5, -1]]), torch.tensor([3, 2]), (1, 2, 3)).tolist() == [2, 3, 4]
    assert rerank.coverage(torch.tensor([[1, 2, 3], [2, 5, -1]]), None, (1, 2, 9)).tolist() == [2, 3, 5]

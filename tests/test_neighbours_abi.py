"""CPU: the C ABI of esr_neighbours.hip -- exported and bound, bad arguments refused with a message before any launch
(stand-in pointers, no device: the technique of test_abi.py), and a plan query that is consistent with itself."""
import ctypes
import os

import pytest

SYMBOLS = ["esr_neighbours_workspace_bytes", "esr_neighbours_plan_bounds", "esr_neighbours_topk",
           "esr_itemknn_max_entries", "esr_itemknn_recommend"]
EINVAL, EWORKSPACE = -1, -3
P = 256   # a stand-in device address: never dereferenced, the calls return before any launch


@pytest.fixture(scope="module")
def lib():
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from esrecsys_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert hasattr(raw, name), "libesr_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def _bounds(lib):
    n = lib.esr_neighbours_plan_bounds(None, 0)
    buf = (ctypes.c_int32 * n)()
    assert lib.esr_neighbours_plan_bounds(ctypes.addressof(buf), n) == n
    return list(buf)


def test_plan_query_is_consistent(lib):
    from esrecsys_amd import ops
    b = _bounds(lib)
    assert len(b) >= 1 and b[0] >= 1
    assert all(x < y for x, y in zip(b, b[1:])), b                  # ascending
    assert b == ops.neighbours_plan_bounds()
    short = (ctypes.c_int32 * 1)(-7)                                # a short buffer is filled as far as it goes
    assert lib.esr_neighbours_plan_bounds(ctypes.addressof(short), 1) == len(b) and short[0] == b[0]
    assert 1 <= lib.esr_itemknn_max_entries() <= 65536 // 12        # key + value per entry in at most 64 KiB of LDS
    assert lib.esr_itemknn_max_entries() == ops.itemknn_max_entries()


def test_workspace_is_monotone_in_the_entry_count(lib):
    ws = lib.esr_neighbours_workspace_bytes
    for both in (0, 1):
        sizes = [ws(n, 1000, both) for n in (0, 1, 63, 64, 65, 1000, 4096, 100_000, 10_000_000)]
        assert sizes[0] > 0 and all(x <= y for x, y in zip(sizes, sizes[1:])), sizes
        assert sizes[-1] >= 10_000_000 * (1 + both) * 12            # a key and a count per listed entry
        assert ws(1000, 10, both) <= ws(1000, 100_000, both)        # and in the ids
    assert all(ws(n, 500, 1) >= ws(n, 500, 0) for n in (0, 10, 5000))
    assert ws(-5, -5, 0) == ws(0, 0, 0)


def test_topk_arguments_are_rejected_without_a_device(lib):
    def topk(nnz=10, u=5, k=10, both=1, score=1, ent=P, ids=P, df=P, out=P, ws=P, ws_bytes=0):
        return lib.esr_neighbours_topk(ent, ent, ent, nnz, ids, df, u, k, both, score, out, out, out, out, ws, ws_bytes,
                                       None)

    def einval(msg, **kw):
        assert topk(**kw) == EINVAL, kw
        err = lib.esr_last_error()
        assert b"esr_neighbours_topk" in err and msg in err, (kw, err)

    assert topk() == EWORKSPACE and b"workspace" in lib.esr_last_error()      # a good call gets as far as the workspace
    for k in (0, -1, 1025):
        einval(b"k=", k=k)
    assert topk(k=1) == EWORKSPACE and topk(k=1024) == EWORKSPACE
    einval(b"bad sizes", nnz=-1)
    einval(b"bad sizes", u=-1)
    einval(b"bad sizes", nnz=1 << 30)
    einval(b"bad sizes", u=1 << 31)
    einval(b"orientation", both=2)
    einval(b"score", score=-1)
    einval(b"no ids", u=0)
    einval(b"null pointer", ws=None, ws_bytes=1 << 40)
    einval(b"null pointer", ids=None)
    einval(b"null pointer", out=None)
    einval(b"null pointer", ent=None)
    einval(b"df", df=None)
    assert topk(df=None, score=0) == EWORKSPACE                                # the count score needs no df
    assert topk(nnz=0, ent=None, df=None) == EWORKSPACE                        # an empty table needs no entries
    assert topk(nnz=0, u=0, ent=None, ids=None, out=None) == 0                 # nothing to do
    need = lib.esr_neighbours_workspace_bytes(10, 5, 1)
    assert topk(ws_bytes=need - 1) == EWORKSPACE
    assert topk(ws=P + 8, ws_bytes=1 << 40) == EWORKSPACE and b"misaligned" in lib.esr_last_error()


def test_recommend_arguments_are_rejected_without_a_device(lib):
    def rec(u=5, width=20, N=10, nq=2, k=10, exclude=1, table=P, hist=P, off=P, out=P):
        return lib.esr_itemknn_recommend(table, table, table, table, u, width, hist, N, off, nq, k, exclude, out, out, out,
                                         None)

    def einval(msg, **kw):
        assert rec(**kw) == EINVAL, kw
        err = lib.esr_last_error()
        assert b"esr_itemknn_recommend" in err and msg in err, (kw, err)

    for k in (0, -3, 1025):
        einval(b"k=", k=k)
    einval(b"width", width=0)
    einval(b"width", width=1025)
    einval(b"bad sizes", u=-1)
    einval(b"bad sizes", N=-1)
    einval(b"bad sizes", nq=-1)
    einval(b"exclude_history", exclude=2)
    einval(b"null pointer", off=None)
    einval(b"null pointer", out=None)
    einval(b"null pointer", hist=None)
    einval(b"null pointer", table=None)
    assert rec(nq=0, off=None, out=None, hist=None, table=None) == 0           # no query: nothing to do

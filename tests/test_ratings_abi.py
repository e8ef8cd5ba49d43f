"""CPU: the C ABI of esr_ratings.hip -- exported and bound, bad arguments refused with a message that carries the function's
name before any launch (stand-in pointers, no device: the technique of test_abi.py), and the two size queries consistent
with ``ops`` and the module."""
import ctypes
import os

import pytest

SYMBOLS = ["esr_usersim_tile", "esr_usersim_table_bytes", "esr_usersim_table_init", "esr_usersim_rehash",
           "esr_usersim_accumulate", "esr_usersim_finalize_workspace_bytes", "esr_usersim_finalize",
           "esr_userknn_max_entries", "esr_userknn_predict", "esr_userknn_recommend"]
EINVAL, EWORKSPACE = -1, -3
P = 256   # a stand-in device address: never dereferenced, the calls return before any launch


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
    from esrecsys_amd import ops, ratings
    T = lib.esr_usersim_tile()
    assert T == ops.usersim_tile() and T >= 2 and T & (T - 1) == 0
    cap = lib.esr_userknn_max_entries()
    assert cap == ops.userknn_max_entries() == ratings.max_entries()
    assert 1 <= cap <= 65536 // 12                                   # key + value per entry in at most 64 KiB of LDS
    tb = lib.esr_usersim_table_bytes
    assert tb(0) == 256 and tb(-4) == 256
    assert [tb(c) for c in (2, 1024, 1 << 20)] == [256 + 40 * c for c in (2, 1024, 1 << 20)]      # a key and four sums
    ws = lib.esr_usersim_finalize_workspace_bytes
    sizes = [ws(n) for n in (0, 1, 255, 256, 257, 100_000, 10_000_000)]
    assert sizes[0] > 0 and all(x <= y for x, y in zip(sizes, sizes[1:])), sizes
    assert ws(-3) == ws(0)


def test_table_arguments_are_rejected_without_a_device(lib):
    init = lambda table=P, capacity=16: lib.esr_usersim_table_init(table, capacity, None)  # noqa: E731
    for c in (0, 1, 3, -8, 48):
        refuses(lib, b"esr_usersim_table_init", init, b"capacity=", capacity=c)
    refuses(lib, b"esr_usersim_table_init", init, b"null (or misaligned) table", table=None)
    refuses(lib, b"esr_usersim_table_init", init, b"null (or misaligned) table", table=P + 8)
    rehash = lambda table=P, capacity=16, new=2 * P, new_capacity=32: lib.esr_usersim_rehash(  # noqa: E731
        table, capacity, new, new_capacity, None)
    refuses(lib, b"esr_usersim_rehash", rehash, b"do not shrink", new_capacity=8)
    refuses(lib, b"esr_usersim_rehash", rehash, b"powers of two", capacity=12)
    refuses(lib, b"esr_usersim_rehash", rehash, b"powers of two", new_capacity=33)
    refuses(lib, b"esr_usersim_rehash", rehash, b"null, misaligned or aliased", table=None)
    refuses(lib, b"esr_usersim_rehash", rehash, b"null, misaligned or aliased", new=None)
    refuses(lib, b"esr_usersim_rehash", rehash, b"null, misaligned or aliased", new=P)
    refuses(lib, b"esr_usersim_rehash", rehash, b"null, misaligned or aliased", new=2 * P + 4)


def test_accumulate_arguments_are_rejected_without_a_device(lib):
    def acc(rat=P, N=10, off=P, ids=P, prefix=P, nitems=4, a=0, b=4, ntiles=4, table=P, capacity=64):
        return lib.esr_usersim_accumulate(rat, rat, N, off, ids, prefix, nitems, a, b, ntiles, table, capacity, None)

    fn = b"esr_usersim_accumulate"
    refuses(lib, fn, acc, b"capacity=", capacity=63)
    refuses(lib, fn, acc, b"negative size", N=-1)
    refuses(lib, fn, acc, b"negative size", nitems=-1)
    refuses(lib, fn, acc, b"negative size", ntiles=-1)
    refuses(lib, fn, acc, b"item range", a=-1)
    refuses(lib, fn, acc, b"item range", a=3, b=2)
    refuses(lib, fn, acc, b"item range", b=5)
    refuses(lib, fn, acc, b"null pointer", table=None)
    refuses(lib, fn, acc, b"null pointer", off=None)
    refuses(lib, fn, acc, b"null pointer", prefix=None)
    refuses(lib, fn, acc, b"null pointer (ratings)", rat=None)
    refuses(lib, fn, acc, b"null pointer (ratings)", ids=None)
    assert acc(a=2, b=2, rat=None, ids=None) == 0                    # an empty range, no ratings, no tile: nothing to do
    assert acc(N=0, rat=None, ids=None) == 0
    assert acc(ntiles=0, rat=None, ids=None) == 0


def test_finalize_arguments_are_rejected_without_a_device(lib):
    def fin(table=P, capacity=64, nnz=10, num_ids=100, min_overlap=1, has_min=0, min_sim=0.0, out=P, counts=P, ws=P,
            ws_bytes=0):
        return lib.esr_usersim_finalize(table, capacity, nnz, num_ids, min_overlap, has_min, min_sim, out, out, out, out,
                                        counts, ws, ws_bytes, None)

    fn = b"esr_usersim_finalize"
    assert fin() == EWORKSPACE and b"workspace" in lib.esr_last_error()        # a good call gets as far as the workspace
    refuses(lib, fn, fin, b"capacity=", capacity=65)
    refuses(lib, fn, fin, b"above 2^31 slots", capacity=1 << 32, nnz=10)
    refuses(lib, fn, fin, b"bad sizes", nnz=-1)
    refuses(lib, fn, fin, b"bad sizes", nnz=65)
    refuses(lib, fn, fin, b"bad sizes", nnz=1 << 30, capacity=1 << 31)
    refuses(lib, fn, fin, b"bad sizes", num_ids=0)
    refuses(lib, fn, fin, b"bad sizes", num_ids=(1 << 31) + 1)
    refuses(lib, fn, fin, b"min_overlap=0", min_overlap=0)
    refuses(lib, fn, fin, b"has_min_similarity=2", has_min=2)
    refuses(lib, fn, fin, b"NaN", has_min=1, min_sim=float("nan"))
    refuses(lib, fn, fin, b"null pointer", table=None)
    refuses(lib, fn, fin, b"null pointer", counts=None)
    refuses(lib, fn, fin, b"null pointer (outputs)", out=None)
    refuses(lib, fn, fin, b"null pointer (outputs)", ws=None, ws_bytes=1 << 40)
    need = lib.esr_usersim_finalize_workspace_bytes(10)
    assert fin(ws_bytes=need - 1) == EWORKSPACE
    assert fin(ws=P + 8, ws_bytes=1 << 40) == EWORKSPACE and b"misaligned" in lib.esr_last_error()
    assert fin(num_ids=1 << 31) == EWORKSPACE                                  # user ids up to 2^31 - 2


def knn_args(table=P, u=5, width=5, users=P, nu=5, off=P, rat=P, R=20, mean=P):
    return (table, table, table, table, u, width, users, nu, off, rat, rat, R, mean)


def shared_refusals(lib, fn, call):
    refuses(lib, fn, call, b"table width=0", width=0)
    refuses(lib, fn, call, b"table width=1025", width=1025)
    for name in ("u", "nu", "R", "nq"):
        refuses(lib, fn, call, b"bad sizes", **{name: -1})
        refuses(lib, fn, call, b"bad sizes", **{name: 1 << 31})
    refuses(lib, fn, call, b"center=2", center=2)
    refuses(lib, fn, call, b"denominator=-1", denominator=-1)
    refuses(lib, fn, call, b"null pointer", q=None)
    refuses(lib, fn, call, b"null pointer", out=None)
    refuses(lib, fn, call, b"null pointer (table)", table=None)
    refuses(lib, fn, call, b"null pointer (ratings)", off=None)
    refuses(lib, fn, call, b"null pointer (ratings)", users=None)
    refuses(lib, fn, call, b"null pointer (ratings)", mean=None)
    refuses(lib, fn, call, b"null pointer (ratings)", rat=None)
    assert call(nq=0, q=None, out=None, table=None, off=None) == 0             # no query: nothing to do


def test_predict_arguments_are_rejected_without_a_device(lib):
    def predict(q=P, nq=3, center=1, denominator=0, out=P, **kw):
        return lib.esr_userknn_predict(*knn_args(**kw), q, q, nq, center, denominator, out, out, None)

    shared_refusals(lib, b"esr_userknn_predict", predict)


def test_recommend_arguments_are_rejected_without_a_device(lib):
    def rec(q=P, nq=3, k=10, exclude=1, min_support=1, center=1, denominator=0, out=P, **kw):
        return lib.esr_userknn_recommend(*knn_args(**kw), q, nq, k, exclude, min_support, center, denominator, out, out,
                                         out, None)

    fn = b"esr_userknn_recommend"
    for k in (0, -3, 1025):
        refuses(lib, fn, rec, b"k=", k=k)
    refuses(lib, fn, rec, b"exclude_rated=2", exclude=2)
    refuses(lib, fn, rec, b"min_support=-1", min_support=-1)
    shared_refusals(lib, fn, rec)

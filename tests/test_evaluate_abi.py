"""CPU: the C ABI of esr_eval.hip -- exported and bound, its caps consistent with ops, and every bad argument refused with
a message that names the entry point before any launch (stand-in pointers, no device: the technique of
test_neighbours_abi.py).  ks is host memory by contract, so the cutoffs here are real arrays."""
import ctypes
import os

import pytest

SYMBOLS = ["esr_eval_max_truth", "esr_eval_max_width", "esr_eval_ranking"]
EINVAL = -1
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


def test_caps_are_consistent(lib):
    from esrecsys_amd import evaluate, ops
    from esrecsys_amd.wikipedia.make_dice import MAX_DOC
    assert lib.esr_eval_max_truth() == ops.eval_max_truth() == evaluate.max_truth() == 4096 == MAX_DOC
    assert lib.esr_eval_max_width() == ops.eval_max_width() == evaluate.max_width() == 4096
    assert 2 * lib.esr_eval_max_truth() * 8 <= 65536               # load <= 1/2 with 8-byte slots: 64 KiB of LDS
    assert evaluate.MAX_CUTOFFS == 8


def test_ranking_arguments_are_rejected_without_a_device(lib):
    def call(ks=(10, 100, 500), nk=None, width=500, pitch=None, nq=4, n=40, max_truth=12, repeats=0, listed=0, rec=P,
             lengths=P, truth=P, off=P, tables=P, out=P, ap=P, fail=P, null_ks=False):
        arr = (ctypes.c_int32 * max(len(ks), 1))(*ks)
        return lib.esr_eval_ranking(rec, width if pitch is None else pitch, width, lengths, truth, n, off, nq, max_truth,
                                    None if null_ks else ctypes.addressof(arr), len(ks) if nk is None else nk, tables,
                                    tables, repeats, listed, out, out, out, out, out, out, ap, ap, fail, None)

    def einval(msg, **kw):
        assert call(**kw) == EINVAL, kw
        err = lib.esr_last_error()
        assert b"esr_eval_ranking" in err and msg in err, (kw, err)

    # the cutoffs
    einval(b"cutoffs", ks=())
    einval(b"cutoffs", ks=tuple(range(1, 10)))                     # nine
    einval(b"cutoffs", null_ks=True)
    einval(b"ascending", ks=(10, 10))
    einval(b"ascending", ks=(100, 10, 500))
    einval(b"ascending", ks=(0, 5))
    einval(b"ascending", ks=(-3,))
    # the sizes
    einval(b"width", width=0)
    einval(b"width", width=4097)
    einval(b"pitch", pitch=499)
    einval(b"bad sizes", nq=-1)
    einval(b"bad sizes", nq=1 << 31)
    einval(b"bad sizes", n=-1)
    einval(b"bad sizes", max_truth=-1)
    einval(b"count_repeats", repeats=2)
    einval(b"truth size", listed=-1)
    # the pointers
    einval(b"null pointer", rec=None)
    einval(b"null pointer", off=None)
    einval(b"null pointer", tables=None)
    einval(b"null pointer", fail=None)
    einval(b"null pointer (truth)", truth=None)
    einval(b"null pointer (outputs)", out=None)
    einval(b"ap, ndcg", ap=None)
    # no query: nothing to do, whatever the pointers -- but the cutoffs and sizes are still checked
    assert call(nq=0, rec=None, lengths=None, truth=None, off=None, tables=None, out=None, ap=None, fail=None) == 0
    assert call(nq=0, ks=(1, 2, 3, 4, 5, 6, 7, 8), width=4096) == 0
    einval(b"ascending", nq=0, ks=(5, 4))
    einval(b"width", nq=0, width=4097)


def test_python_refuses_before_any_device_is_touched():
    """ranking_metrics' argument checks that need no device: the cutoffs, the size mode and CPU lists"""
    import torch
    from esrecsys_amd.evaluate import ranking_metrics
    rec = torch.zeros((2, 4), dtype=torch.int32)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ranking_metrics(rec, None, [1, 2], [0, 1, 2])
    with pytest.raises(ValueError, match="ascending"):
        ranking_metrics(rec, None, [1, 2], [0, 1, 2], ks=(10, 5))
    with pytest.raises(ValueError, match="9 cutoffs"):
        ranking_metrics(rec, None, [1, 2], [0, 1, 2], ks=range(1, 10))
    with pytest.raises(ValueError, match="truth_size"):
        ranking_metrics(rec, None, [1, 2], [0, 1, 2], truth_size="unique")

"""CPU: the co-occurrence builder's host side -- the two restatements of the window rule agree, the line-file writer
round-trips through the project's readers, splits rows as the reference does and emits the bytes protobuf's serialiser
emits, and the esr_cooccur_* entry points reject bad arguments before touching a device."""
import base64
import os

import numpy as np
import pytest

from _cooccur_ref import lcm_upto, ref_exact, ref_float, ulp_distance, zipf_docs
from conftest import GOLDEN

from esrecsys_amd.wikipedia import make_cooccurrence as mc
from esrecsys_amd.wikipedia.cooccurrence_matrix import CooccurrenceGenerator, CooccurrenceMatrix, decode_lines


def test_lcm_leaves_room_in_a_uint64_sum():
    assert lcm_upto(10) == 2520 and lcm_upto(22) == 232_792_560 < 2 ** 28
    assert lcm_upto(23) > 2 ** 28   # why the window stops at 22


def test_hand_worked_window_is_asymmetric():
    """W = 2, t = [5, 1, 4, 2, 3]: position i sees j in {i - 2, i - 1, i + 1} (W back, W - 1 forward).
    i=0 (5): j=1 -> (5,1) += 1.            i=1 (1): nothing is smaller.
    i=2 (4): j=1 -> (4,1) += 1; j=3 -> (4,2) += 1.       (j=0: 5 is larger)
    i=3 (2): j=1 -> (2,1) += 1/2.          (j=2, j=4 larger)
    i=4 (3): j=3 -> (3,2) += 1.            (j=2 larger)
    NOT there: (5,4) -- 5 at i=0 would have to look 2 FORWARD -- and (4,3), 4 at i=2 looking 2 forward."""
    index, other, count = ref_exact([[5, 1, 4, 2, 3]], 2)
    assert list(zip(index.tolist(), other.tolist(), count.tolist())) == \
        [(2, 1, 0.5), (3, 2, 1.0), (4, 1, 1.0), (4, 2, 1.0), (5, 1, 1.0)]
    # the mirrored document: the larger id now looks BACK two positions, so those pairs appear with 1/2
    index, other, count = ref_exact([[3, 2, 4, 1, 5]], 2)
    got = dict(zip(zip(index.tolist(), other.tolist()), count.tolist()))
    assert got[(5, 4)] == 0.5 and got[(4, 3)] == 0.5


@pytest.mark.parametrize("W", [1, 2, 10, 22])
@pytest.mark.parametrize("V", [3, 50, 5000])
def test_float_and_exact_restatements_agree_to_one_ulp(W, V):
    """ref_float carries a relative error of at most n * 2^-53 after n adds of correctly rounded 1/d -- far below half an
    f32 ulp (2^-25) for any n reached here -- so after the rounding to f32 the two can differ only where the exact sum
    sits at a rounding tie: at most 1 ulp."""
    docs = zipf_docs(np.random.default_rng(1000 * W + V), 60, V, 399)
    fi, fo, fc = ref_float(docs, W)
    ei, eo, ec = ref_exact(docs, W)
    assert np.array_equal(fi, ei) and np.array_equal(fo, eo)
    d = ulp_distance(fc, ec)
    print("W=%d V=%d pairs=%d max ulp=%d" % (W, V, len(ec), d.max() if len(d) else 0))
    assert len(ec) > 0 and d.max() <= 1


def _entries(rng, row_sizes, max_id=2 ** 31 - 1):
    index, other, count = [], [], []
    idx = 0
    for n in row_sizes:
        idx += int(rng.integers(1, 1000))
        index += [idx] * n
        other += sorted(int(x) for x in rng.choice(max(idx, n + 1) if idx < 10 ** 6 else 10 ** 6, n, replace=False))
        count += [float(np.float32(c)) for c in rng.uniform(1 / 22, 3000.0, n)]
    return np.array(index, np.int32), np.array(other, np.int32), np.array(count, np.float32)


def test_writer_round_trips_bit_for_bit(tmp_path):
    rng = np.random.default_rng(3)
    index, other, count = _entries(rng, [1, 7, 130, 1, 2, 40])
    index[-1] = index[-2] = 2 ** 31 - 1   # a wide index: the last row is now two rows
    path = str(tmp_path / "m.cooccur.pb.b64.bz2")
    lines = mc.write_cooccurrence(path, index, other, count)
    assert lines == 7
    gen = CooccurrenceGenerator(path).get_item()
    items = [next(gen) for _ in range(len(index))]
    assert [i[0] for i in items] == index.tolist() and [i[1] for i in items] == other.tolist()
    assert np.array_equal(np.array([i[2] for i in items], np.float32).view(np.int32), count.view(np.int32))
    assert next(gen)[:2] == (int(index[0]), int(other[0]))   # cycles
    import bz2
    t1, t2, cnt, used = decode_lines(bz2.open(path, "rb").read())
    assert np.array_equal(t1, index) and np.array_equal(t2, other)
    assert np.array_equal(cnt.view(np.int32), count.view(np.int32))


@pytest.mark.parametrize("max_row_size,n,pieces", [
    (1000, 1000, [1000]), (1000, 1001, [1001]), (1000, 1002, [1001, 1]), (1000, 2003, [1001, 1001, 1]),
    (1, 1000, [2] * 500), (1, 1001, [2] * 500 + [1]), (1, 1002, [2] * 501), (1, 2003, [2] * 1001 + [1])])
def test_row_split_keeps_the_references_off_by_one(tmp_path, max_row_size, n, pieces):
    """A row is cut when len(count) > max_row_size AFTER an append: full pieces hold max_row_size + 1 entries."""
    rng = np.random.default_rng(n)
    index, other, count = _entries(rng, [3, n, 2])
    path = str(tmp_path / "split.cooccur.pb.b64.bz2")
    mc.write_cooccurrence(path, index, other, count, max_row_size=max_row_size)
    import bz2
    rows = [mc_row for mc_row in bz2.open(path, "rb").read().split(b"\n") if mc_row]
    from esrecsys_amd.wikipedia.cooccurrence_matrix import parse_cooccurrence_row
    parsed = [parse_cooccurrence_row(base64.b64decode(r)) for r in rows]
    big = int(index[3])
    assert [len(p[1]) for p in parsed if p[0] == big] == pieces
    assert all(len(p[1]) == len(p[2]) and 0 < len(p[1]) <= max_row_size + 1 for p in parsed)
    # the matrix consumer appends the repeated row indices back into one row
    m = CooccurrenceMatrix(path).rows()
    assert sorted(m) == sorted(set(index.tolist()))
    got = m[big]
    assert [o for o, _ in got] == other[3:3 + n].tolist()
    assert np.array_equal(np.array([c for _, c in got], np.float32).view(np.int32), count[3:3 + n].view(np.int32))


def test_encoder_emits_the_protobuf_serialisers_bytes():
    """tests/golden/writer_rows.*: rows and the lines the reference's generated nlp_pb2.CooccurrenceRow serialises for them
    (tests/golden/make_cooccur_writer_fixture.py) -- ids of every varint width up to 2^31 - 1, a large index, empty rows."""
    with np.load(os.path.join(GOLDEN, "writer_rows.npz")) as z:
        row_index, row_start, other, count = z["row_index"], z["row_start"], z["other"], z["count"]
    want = open(os.path.join(GOLDEN, "writer_rows.b64.txt"), "rb").read().split(b"\n")[:-1]
    assert len(want) == len(row_index) >= 20
    assert other.max() >= 2 ** 28 and row_index.max() == 2 ** 31 - 1
    for width in (2 ** 7, 2 ** 14, 2 ** 21, 2 ** 28):
        assert (other >= width).any() and (other < width).any()
    for r, line in enumerate(want):
        a, b = row_start[r], row_start[r + 1]
        assert base64.b64encode(mc.encode_cooccurrence_row(row_index[r], other[a:b], count[a:b])) == line, r


def test_pack_docs_makes_csr_with_empty_documents():
    tokens, off = mc.pack_docs([[], [3, 1], [], [7], []])
    assert tokens.tolist() == [3, 1, 7] and tokens.dtype == np.int32
    assert off.tolist() == [0, 0, 2, 2, 3, 3] and off.dtype == np.int64
    tokens, off = mc.pack_docs([])
    assert tokens.size == 0 and off.tolist() == [0]


def test_cooccur_arguments_are_rejected_without_a_device():
    """Stand-in (non-null, aligned) pointers, never dereferenced: every call returns before any launch."""
    from esrecsys_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from esrecsys_amd.build import build_library
        build_library()
    lib = _lib.load()
    EINVAL = -1
    P = 256

    def acc(tokens=P, N=100, off=P, ndocs=3, a=0, b=100, W=10, table=P, cap=1024):
        return lib.esr_cooccur_accumulate(tokens, N, off, ndocs, a, b, W, table, cap, None)

    for W in (0, 23, -1):
        assert acc(W=W) == EINVAL and b"context_window" in lib.esr_last_error()
    for cap in (0, 1, 3, 1000, -8):
        assert acc(cap=cap) == EINVAL and b"power of two" in lib.esr_last_error()
    assert acc(N=-1, b=0) == EINVAL and b"negative size" in lib.esr_last_error()
    assert acc(ndocs=-1) == EINVAL
    for a, b in ((-1, 10), (10, 5), (0, 101)):
        assert acc(a=a, b=b) == EINVAL and b"token range" in lib.esr_last_error()
    assert acc(table=None) == EINVAL and b"null pointer" in lib.esr_last_error()
    assert acc(off=None) == EINVAL
    assert acc(tokens=None) == EINVAL
    assert acc(a=40, b=40) == 0 and acc(ndocs=0) == 0      # nothing to do: no launch

    assert lib.esr_cooccur_table_init(P, 12, None) == EINVAL and b"power of two" in lib.esr_last_error()
    assert lib.esr_cooccur_table_init(None, 16, None) == EINVAL
    assert lib.esr_cooccur_rehash(P, 16, 512, 8, None) == EINVAL     # shrinking
    assert lib.esr_cooccur_rehash(P, 16, 512, 24, None) == EINVAL
    assert lib.esr_cooccur_rehash(P, 16, P, 32, None) == EINVAL and b"aliased" in lib.esr_last_error()
    assert lib.esr_cooccur_rehash(None, 16, 512, 32, None) == EINVAL

    def fin(W=10, cap=1024, nnz=10, V=100, out=P, ws=P, ws_bytes=1 << 30):
        return lib.esr_cooccur_finalize(P, cap, nnz, V, W, out, out, out, ws, ws_bytes, None)

    assert fin(W=0) == EINVAL and fin(W=23) == EINVAL
    assert fin(cap=1000) == EINVAL
    assert fin(nnz=-1) == EINVAL and fin(nnz=1025) == EINVAL and b"bad sizes" in lib.esr_last_error()
    assert fin(V=0) == EINVAL and fin(V=2 ** 31 + 1) == EINVAL
    assert fin(out=None) == EINVAL and fin(ws=None) == EINVAL
    assert fin(nnz=0, out=None, ws=None) == 0
    assert fin(ws_bytes=lib.esr_cooccur_finalize_workspace_bytes(10) - 1) == -3
    assert lib.esr_cooccur_table_bytes(1024) == 256 + 16 * 1024
    assert lib.esr_cooccur_finalize_workspace_bytes(1 << 20) > lib.esr_cooccur_finalize_workspace_bytes(1 << 10) > 0


def test_builder_refuses_unsupported_windows():
    for W in (0, 23):
        with pytest.raises(ValueError, match="context_window"):
            mc.CooccurrenceBuilder(context_window=W)

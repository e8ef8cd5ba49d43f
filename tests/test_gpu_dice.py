"""GPU: the Dice builder (esr_dice.hip, wikipedia/make_dice.py) against the CPU restatement of the set-pair rule -- index,
other and count BIT FOR BIT (the sums are integers: nothing depends on atomic order or on how the work is cut), and the
document frequencies exactly.

The reference's make_dice.py imports PySpark at its top and cannot be run here: parity rests on its source text
(make_dice.py:41-54: set, sort, every i < j adds 1 to (u[i], u[j])), restated twice in tests/_dice_ref.py;
test_dice_host.py holds the two restatements against each other on the inputs used here."""
import numpy as np
import pytest
import torch

from _dice_ref import BIG, MAX_DOC, SIZES, case_docs, case_ref

from esrecsys_amd.wikipedia import make_dice as md

pytestmark = pytest.mark.gpu


def _host(result):
    return tuple(x.cpu().numpy() for x in result)


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def _check(builder, name):
    """finalize() and doc_frequency() of the builder against the case's restatement."""
    ei, eo, ec, eids, edf = case_ref(name)
    index, other, count = _host(builder.finalize())
    assert index.dtype == np.int32 and other.dtype == np.int32 and count.dtype == np.float32
    assert len(index) == len(ei) == builder.nnz, "nnz %d, reference %d" % (len(index), len(ei))
    assert np.array_equal(index.astype(np.int64), ei) and np.array_equal(other.astype(np.int64), eo)
    assert np.array_equal(count.view(np.int32), ec.view(np.int32))
    assert np.all(index < other)
    ids, df = _host(builder.doc_frequency())
    assert ids.dtype == np.int32 and df.dtype == np.float32
    assert np.array_equal(ids.astype(np.int64), eids) and np.array_equal(df.view(np.int32), edf.view(np.int32))
    return index, other, count


def _build(name, dev, **kw):
    b = md.DiceBuilder(device=dev, **kw)
    b.add(*md.pack_docs(case_docs(name)))
    return b


@pytest.mark.parametrize("n", SIZES)
def test_document_sizes(dev, n):
    """Around the wave path's 64 ids, the workgroup sort's sizes (256, and the next power of two above 257 and 1025), one
    triangle tile and many, the cap and one below it."""
    _check(_build("size_%d" % n, dev, capacity=64), "size_%d" % n)


def test_full_triangle_at_the_cap(dev):
    """MAX_DOC distinct ids: 8.4 M pairs over 256 triangle tiles, each once.  The expectation is the rule itself in closed
    form (every i < j of the sorted ids; test_dice_host.py holds it against the restatement at 300 ids) -- the pure-Python
    double loop over this one document takes tens of seconds."""
    from _dice_ref import full_triangle_doc
    doc, ei, eo = full_triangle_doc()
    b = md.DiceBuilder(capacity=64, device=dev)
    b.add(doc, np.array([0, MAX_DOC], np.int64))
    index, other, count = b.finalize()
    assert b.nnz == MAX_DOC * (MAX_DOC - 1) // 2 == index.numel()
    assert torch.equal(index.cpu().to(torch.int64), torch.from_numpy(ei))
    assert torch.equal(other.cpu().to(torch.int64), torch.from_numpy(eo))
    assert bool((count == 1).all())
    ids, df = b.doc_frequency()
    assert np.array_equal(ids.cpu().numpy(), np.sort(doc)) and bool((df == 1).all())


def test_one_id_repeated_yields_no_pairs(dev):
    b = _build("one_id_repeated", dev, capacity=8)
    _check(b, "one_id_repeated")
    assert b.nnz == 0 and b.finalize()[0].numel() == 0 and b.doc_frequency()[0].tolist() == [3, 5, 7, 8, 9]


def test_primary_repeated_among_the_secondaries(dev):
    index, other, count = _check(_build("primary_repeated", dev, capacity=8), "primary_repeated")
    assert list(zip(index.tolist(), other.tolist(), count.tolist())) == \
        [(1, 2, 1.0), (2, 4, 1.0), (2, 9, 1.0), (4, 9, 1.0), (5, 6, 1.0)]


def test_ids_zero_and_largest(dev):
    index, other, _ = _check(_build("extreme_ids", dev, capacity=4), "extreme_ids")
    assert index.min() == 0 and other.max() == BIG and (index == BIG - 1).any()


def test_contention_on_one_pair_is_exact(dev):
    """3000 two-id documents of the same pair: every increment lands on one key (and two diagonal ones)."""
    index, other, count = _check(_build("contention_3000", dev, capacity=8), "contention_3000")
    assert (index.tolist(), other.tolist(), count.tolist()) == ([5], [11], [3000.0])


def test_many_tiny_documents_inside_one_wave(dev):
    _check(_build("tiny_docs_in_a_wave", dev, capacity=16), "tiny_docs_in_a_wave")


def test_no_documents(dev):
    b = md.DiceBuilder(capacity=8, device=dev)
    b.add(np.zeros(0, np.int32), np.zeros(1, np.int64))
    b.add(np.zeros(0, np.int32), np.zeros(4, np.int64))      # three empty documents
    index, other, count = b.finalize()
    assert b.nnz == 0 and index.numel() == other.numel() == count.numel() == 0 and index.is_cuda
    assert b.doc_frequency()[0].numel() == 0
    assert md.process_sdocs([], device=dev)[0].numel() == 0


def test_cut_invariance(dev):
    """One add; the same corpus over several add calls (device inputs); max_pairs_per_launch small from capacity 2, which
    forces many launches and rehashes: identical tensors, all equal to the restatement."""
    docs = case_docs("cut_corpus")
    one = _build("cut_corpus", dev)
    _check(one, "cut_corpus")
    assert one.launches == 1
    whole = _host(one.finalize()) + _host(one.doc_frequency())

    several = md.DiceBuilder(capacity=1 << 10, device=dev)
    cuts = [0, 1, 4, 5, 230, 231, 900, len(docs)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        indices, off = md.pack_docs(docs[lo:hi])
        several.add(torch.from_numpy(indices).to(dev), torch.from_numpy(off).to(dev))
    _assert_same(_host(several.finalize()) + _host(several.doc_frequency()), whole)

    small = md.DiceBuilder(capacity=2, device=dev, max_pairs_per_launch=3000)
    small.add(*md.pack_docs(docs))
    assert small.launches > 50 and small.rehashes >= 5 and small.capacity >= 2 * small.nnz
    _assert_same(_host(small.finalize()) + _host(small.doc_frequency()), whole)

    # finalize leaves the builder usable: the same documents again double every count and every frequency
    one.add(*md.pack_docs(docs))
    twice = _host(one.finalize()) + _host(one.doc_frequency())
    assert np.array_equal(twice[0], whole[0]) and np.array_equal(twice[1], whole[1]) and np.array_equal(twice[3], whole[3])
    assert np.array_equal(twice[2], 2 * whole[2]) and np.array_equal(twice[4], 2 * whole[4])


def test_dice_scores(dev):
    """joint / (df[other] + df[index]), no factor 2 (dump_dice.py:36-45): within 1e-6 relative of float64 (one f32 add and
    one f32 division of exactly represented integers: 2^-23 = 1.2e-7 at most)."""
    b = _build("cut_corpus", dev)
    index, other, count = b.finalize()
    ids, df = b.doc_frequency()
    scores = md.dice_scores(index, other, count, ids, df)
    assert scores.dtype == torch.float32 and scores.shape == count.shape and scores.is_cuda
    ei, eo, ec, eids, edf = case_ref("cut_corpus")
    freq = dict(zip(eids.tolist(), edf.astype(np.float64).tolist()))
    want = np.array([c / (freq[o] + freq[i]) for i, o, c in zip(ei.tolist(), eo.tolist(), ec.astype(np.float64).tolist())])
    rel = np.abs(scores.cpu().numpy().astype(np.float64) - want) / want
    print("dice_scores: max relative error %.3g over %d entries" % (rel.max(), len(want)))
    assert rel.max() <= 1e-6 and 0 < want.min() and want.max() <= 0.5


@pytest.mark.parametrize("n", [3, 100])
def test_negative_id_raises_and_leaves_the_builder_unusable(dev, n):
    """A negative id in a device tensor (not screened on the host), on the wave path (3 ids) and on the workgroup path
    (100 ids), raises the table's failure word.  The kernels use an id only as a sort key and as half of a hash key --
    never as an address -- and skip the whole document."""
    ids = np.arange(n, dtype=np.int32)
    ids[n // 2] = -1
    b = md.DiceBuilder(capacity=8, device=dev)
    with pytest.raises(md.CooccurrenceError, match="negative id"):
        b.add(torch.from_numpy(ids).to(dev), np.array([0, n], np.int64))
    for call in (lambda: b.add(np.array([1, 2], np.int32), np.array([0, 2], np.int64)), b.finalize, b.doc_frequency,
                 lambda: b.nnz):
        with pytest.raises(md.CooccurrenceError, match="unusable"):
            call()


def test_document_above_the_cap_is_refused(dev):
    b = md.DiceBuilder(capacity=8, device=dev)
    with pytest.raises(ValueError, match="document 0 holds %d ids" % (MAX_DOC + 1)):
        b.add(torch.zeros(MAX_DOC + 1, dtype=torch.int32, device=dev), np.array([0, MAX_DOC + 1], np.int64))
    b.add(np.array([2, 1], np.int32), np.array([0, 2], np.int64))      # the builder is still sound
    assert [x.tolist() for x in b.finalize()] == [[1], [2], [1.0]]


def test_written_file_reads_back_and_a_row_of_1002_splits(dev, tmp_path):
    """write_cooccurrence -> the project's own reader returns the same entries; the reference's
    `len(proto.count) > max_row_size` rule cuts the row of 1002 entries into 1001 + 1."""
    import base64
    import bz2
    from esrecsys_amd.wikipedia.cooccurrence_matrix import CooccurrenceGenerator, parse_cooccurrence_row
    index, other, count = md.process_sdocs(case_docs("row_of_1002"), device=dev)
    ei, eo, ec, _, _ = case_ref("row_of_1002")
    hi, ho, hc = _host((index, other, count))
    assert np.array_equal(hi.astype(np.int64), ei) and np.array_equal(ho.astype(np.int64), eo) and np.array_equal(hc, ec)
    path = str(tmp_path / "dice.cooccur.pb.b64.bz2")
    lines = md.write_cooccurrence(path, index, other, count, max_row_size=md.FLAGS.max_row_size)
    rows = [parse_cooccurrence_row(base64.b64decode(r)) for r in bz2.open(path, "rb").read().split(b"\n") if r]
    assert len(rows) == lines and [len(r[1]) for r in rows if r[0] == 0] == [1001, 1]
    nnz = len(ei)
    (t1, t2), cnt = next(CooccurrenceGenerator(path).get_batch(nnz))
    assert sorted(zip(t1.tolist(), t2.tolist(), cnt.view(np.int32).tolist())) == \
        sorted(zip(ei.tolist(), eo.tolist(), ec.view(np.int32).tolist()))


def test_main_writes_the_line_file(dev, tmp_path):
    from esrecsys_amd.wikipedia.cooccurrence_matrix import CooccurrenceGenerator
    indices, off = md.pack_docs(case_docs("primary_repeated"))
    src, dst = str(tmp_path / "in.npz"), str(tmp_path / "out.cooccur.pb.b64.bz2")
    np.savez(src, indices=indices, doc_offsets=off)
    md.main(["--input_file", src, "--output_file", dst])
    (t1, t2), cnt = next(CooccurrenceGenerator(dst).get_batch(5))
    assert sorted(zip(t1.tolist(), t2.tolist(), cnt.tolist())) == \
        [(1, 2, 1.0), (2, 4, 1.0), (2, 9, 1.0), (4, 9, 1.0), (5, 6, 1.0)]


def test_device_batches_feed_a_train_step(dev):
    """device_batches accepts the result unchanged and feeds one train_epoch step."""
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.wikipedia.models import Glove
    from esrecsys_amd.wikipedia.train_cooccurence import train_epoch
    index, other, count = _build("cut_corpus", dev).finalize()
    B = 256
    assert index.numel() > B
    it = md.device_batches(index, other, count, B, generator=torch.Generator(device=dev).manual_seed(3))
    x, y = next(it)
    assert x.is_cuda and x.dtype == torch.int32 and x.shape == (2, B) and y.dtype == torch.float32 and y.shape == (B,)
    assert bool((x[0] < x[1]).all())
    model = Glove(num_embeddings=5000, features=16, device=dev)
    state = TrainState.create(apply_fn=model.apply, params=model.init(7, None)["params"], tx=optim.sparse_adagrad(0.05))
    losses = []
    state, loss = train_epoch(state, 1, iter([(x, y)]), losses_out=losses)
    assert np.isfinite(loss) and bool(torch.isfinite(losses[0]).all())

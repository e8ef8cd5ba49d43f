"""GPU: the co-occurrence builder (esr_cooccur.hip, wikipedia/make_cooccurrence.py) against the CPU restatement of the
window rule -- index, other and count BIT FOR BIT against ref_exact (the sums are integers: nothing depends on atomic
order or chunking) and within 1 f32 ulp of ref_float (the reference's fp64 adds; see test_cooccur_host.py for the bound)."""
import numpy as np
import pytest
import torch

from _cooccur_ref import lcm_upto, ref_exact, ref_float, ulp_distance, zipf_docs

from esrecsys_amd.wikipedia import make_cooccurrence as mc

pytestmark = pytest.mark.gpu


def _host(result):
    return tuple(x.cpu().numpy() for x in result)


def _assert_same(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def _check(result, docs, W, float_too=True):
    index, other, count = _host(result)
    assert index.dtype == np.int32 and other.dtype == np.int32 and count.dtype == np.float32
    ei, eo, ec = ref_exact(docs, W)
    assert len(index) == len(ei), "nnz %d, reference %d" % (len(index), len(ei))
    assert np.array_equal(index.astype(np.int64), ei) and np.array_equal(other.astype(np.int64), eo)
    assert np.array_equal(count.view(np.int32), ec.view(np.int32))
    composite = (index.astype(np.int64) << 32) | other.astype(np.int64)
    assert np.all(np.diff(composite) > 0)           # strictly ascending (index, other)
    if float_too and len(ei):
        fi, fo, fc = ref_float(docs, W)
        assert np.array_equal(fi, ei) and np.array_equal(fo, eo) and ulp_distance(count, fc).max() <= 1
    return index, other, count


def _build(docs, W, dev, **kw):
    b = mc.CooccurrenceBuilder(W, device=dev, **kw)
    b.add(*mc.pack_docs(docs))
    return b, b.finalize()


@pytest.mark.parametrize("W", [1, 2, 10, 22])
def test_window_edges(dev, W):
    """Documents around the window: 0, 1, 2, W - 1, W, W + 1, 2W, 2W + 1 tokens, few distinct ids (repeats inside a
    window) and many (every pair its own key)."""
    rng = np.random.default_rng(W)
    lengths = [0, 1, 2, max(W - 1, 0), W, W + 1, 2 * W, 2 * W + 1]
    docs = [rng.integers(0, 7, n).astype(np.int32) for n in lengths] + \
           [rng.integers(0, 100000, n).astype(np.int32) for n in lengths]
    b, res = _build(docs, W, dev, capacity=64)
    _check(res, docs, W)
    assert b.nnz == res[0].numel()


def test_hand_worked_asymmetric_window(dev):
    """W = 2, [5, 1, 4, 2, 3]: W back, W - 1 forward (worked out in test_cooccur_host.py)."""
    index, other, count = _host(mc.process_docs([[5, 1, 4, 2, 3]], context_window=2, device=dev))
    assert list(zip(index.tolist(), other.tolist(), count.tolist())) == \
        [(2, 1, 0.5), (3, 2, 1.0), (4, 1, 1.0), (4, 2, 1.0), (5, 1, 1.0)]
    index, other, count = _host(mc.process_docs([[3, 2, 4, 1, 5]], context_window=2, device=dev))
    got = dict(zip(zip(index.tolist(), other.tolist()), count.tolist()))
    assert got[(5, 4)] == 0.5 and got[(4, 3)] == 0.5 and len(got) == 6


def test_document_boundaries(dev):
    """Many short documents back to back (no pair may cross an offset), empty ones at the start, in the middle, at the end."""
    rng = np.random.default_rng(5)
    docs = [[], []] + [rng.integers(0, 40, int(rng.integers(0, 4))).astype(np.int32) for _ in range(700)] + [[]]
    docs[300] = []
    docs[301] = []
    _check(_build(docs, 10, dev, capacity=16)[1], docs, 10)
    # cut inside documents too: a launch covers 3 positions
    _check(_build(docs, 10, dev, capacity=16, max_pairs_per_launch=30 * 10)[1], docs, 10)


def test_no_documents(dev):
    b = mc.CooccurrenceBuilder(10, capacity=8, device=dev)
    b.add(np.zeros(0, np.int32), np.zeros(1, np.int64))
    b.add(np.zeros(0, np.int32), np.zeros(4, np.int64))      # three empty documents
    index, other, count = b.finalize()
    assert b.nnz == 0 and index.numel() == other.numel() == count.numel() == 0 and index.is_cuda
    assert mc.process_docs([], device=dev)[0].numel() == 0


def test_equal_ids_never_pair(dev):
    b, res = _build([[4] * 300], 10, dev, capacity=8)
    assert b.nnz == 0 and res[0].numel() == 0
    docs = [[9, 2] * 150]
    index, other, count = _check(_build(docs, 10, dev, capacity=8)[1], docs, 10)
    assert index.tolist() == [9] and other.tolist() == [2] and count[0] > 300


def test_contention_is_exact_and_repeatable(dev):
    """200 000 tokens over three ids: every increment lands on one of three keys."""
    W = 4
    docs = [np.random.default_rng(9).integers(0, 3, 200_000).astype(np.int32)]
    first = _check(_build(docs, W, dev, capacity=8)[1], docs, W)
    assert len(first[0]) == 3
    _assert_same(first, _host(_build(docs, W, dev, capacity=8)[1]))


def test_full_width_keys(dev):
    """Ids up to 2^31 - 1 beside small ones; keys that agree in their high half, in their low half, and one key's high
    half as another's low half."""
    big = 2 ** 31 - 1
    docs = [[big, 5], [6, big], [7, 5], [5, big - 1], [100, 7], [2 ** 30, 100], [big, big - 1, 0, 2 ** 30],
            [65536, 1], [1, 65537], [big, 2 ** 16, big, 3]]
    index, other, _ = _check(_build(docs, 10, dev, capacity=4)[1], docs, 10)
    assert index.max() == big and (other == big - 1).any()


@pytest.fixture(scope="module")
def corpus():
    """~ 50 000 distinct pairs (W = 22), shared by the growth and chunking tests with its reference."""
    docs = zipf_docs(np.random.default_rng(22), 70, 20000, 200, a=1.2)
    return docs, 22, ref_exact(docs, 22)


def test_growth_from_the_smallest_table(dev, corpus):
    """capacity 2 and launches of at most 4096 pairs: the table is rehashed many times inside and between add calls; the
    result is the roomy table's, bit for bit."""
    docs, W, (ei, eo, ec) = corpus
    assert 40_000 < len(ei)
    roomy, want = _build(docs, W, dev, capacity=1 << 18)
    assert roomy.rehashes == 0
    b = mc.CooccurrenceBuilder(W, capacity=2, device=dev, max_pairs_per_launch=4096)
    for part in (docs[:20], docs[20:45], docs[45:]):
        b.add(*mc.pack_docs(part))
    assert b.rehashes >= 5 and b.capacity >= 2 * b.nnz and b.nnz == len(ei)
    got = _host(b.finalize())
    _assert_same(got, _host(want))
    assert np.array_equal(got[0].astype(np.int64), ei) and np.array_equal(got[1].astype(np.int64), eo)
    assert np.array_equal(got[2].view(np.int32), ec.view(np.int32))


def test_chunking_and_document_order_do_not_matter(dev, corpus):
    docs, W, (ei, eo, ec) = corpus
    whole = _host(_build(docs, W, dev)[1])
    assert np.array_equal(whole[2].view(np.int32), ec.view(np.int32)) and np.array_equal(whole[0].astype(np.int64), ei)
    b = mc.CooccurrenceBuilder(W, capacity=1 << 10, device=dev)
    cuts = [0, 1, 4, 5, 23, 24, 51, len(docs)]                   # seven uneven add calls
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        tokens, off = mc.pack_docs(docs[lo:hi])
        b.add(torch.from_numpy(tokens).to(dev), torch.from_numpy(off).to(dev))   # device inputs
    _assert_same(_host(b.finalize()), whole)
    _assert_same(_host(_build(docs[::-1], W, dev)[1]), whole)
    # finalize leaves the builder usable: the same documents again double every sum
    b.add(*mc.pack_docs(docs))
    twice = _host(b.finalize())
    assert np.array_equal(twice[0], whole[0]) and np.array_equal(twice[1], whole[1])
    L = lcm_upto(W)
    sums = np.rint(whole[2].astype(np.float64) * L)              # (exact only where the sum fits f32: compare loosely)
    assert np.allclose(twice[2], np.float32(2 * sums / L), rtol=1e-6)


def test_failure_flag_becomes_an_exception(dev):
    """A negative id (device tensors are not screened on the host) raises the table's failure word: the add raises and
    the builder refuses further work."""
    b = mc.CooccurrenceBuilder(2, capacity=8, device=dev)
    with pytest.raises(mc.CooccurrenceError, match="negative token id"):
        b.add(torch.tensor([3, -1, 2], dtype=torch.int32, device=dev), np.array([0, 3], np.int64))
    with pytest.raises(mc.CooccurrenceError, match="unusable"):
        b.add(np.array([1, 2], np.int32), np.array([0, 2], np.int64))
    with pytest.raises(mc.CooccurrenceError, match="unusable"):
        b.finalize()
    with pytest.raises(ValueError, match="doc_offsets"):
        mc.CooccurrenceBuilder(2, capacity=8, device=dev).add(np.array([1, 2], np.int32), np.array([0, 3], np.int64))


def test_end_to_end_file_batches_and_training(dev, tmp_path):
    """process_docs -> write_cooccurrence -> the existing reader returns the same multiset; device_batches covers every
    entry once per pass and feeds train_epoch: three steps, finite loss, equal to the same batches fed as host arrays."""
    from esrecsys_amd import TrainState, optim
    from esrecsys_amd.wikipedia.cooccurrence_matrix import CooccurrenceGenerator
    from esrecsys_amd.wikipedia.models import Glove
    from esrecsys_amd.wikipedia.train_cooccurence import train_epoch
    V, W, B = 300, 10, 128
    docs = zipf_docs(np.random.default_rng(4), 30, V, 120)
    index, other, count = mc.process_docs(docs, context_window=W, device=dev)
    hi, ho, hc = _check((index, other, count), docs, W)
    nnz = len(hi)
    assert nnz > 2 * B
    path = str(tmp_path / "e2e.cooccur.pb.b64.bz2")
    mc.write_cooccurrence(path, index, other, count, max_row_size=50)
    (t1, t2), cnt = next(CooccurrenceGenerator(path).get_batch(nnz))
    want = sorted(zip(hi.tolist(), ho.tolist(), hc.view(np.int32).tolist()))
    assert sorted(zip(t1.tolist(), t2.tolist(), cnt.view(np.int32).tolist())) == want

    g = torch.Generator(device=dev).manual_seed(5)
    it = mc.device_batches(index, other, count, B, generator=g)
    npass = -(-nnz // B)
    batches = [next(it) for _ in range(2 * npass)]
    for x, y in batches:
        assert x.is_cuda and x.dtype == torch.int32 and x.shape == (2, B) and x.is_contiguous()
        assert y.is_cuda and y.dtype == torch.float32 and y.shape == (B,)
    xs = torch.cat([x for x, _ in batches], 1).cpu().numpy()
    ys = torch.cat([y for _, y in batches]).cpu().numpy().view(np.int32)
    for p in range(2):                                           # every entry exactly once per pass
        sl = slice(p * nnz, (p + 1) * nnz)
        assert sorted(zip(xs[0, sl].tolist(), xs[1, sl].tolist(), ys[sl].tolist())) == want
    assert not np.array_equal(xs[:, :nnz], xs[:, nnz:2 * nnz])   # a fresh permutation per pass

    def run(feed):
        model = Glove(num_embeddings=V, features=16, device=dev)
        state = TrainState.create(apply_fn=model.apply, params=model.init(7, None)["params"], tx=optim.sparse_adagrad(0.05))
        losses = []
        state, loss = train_epoch(state, 3, iter(feed), losses_out=losses)
        return loss, losses[0].cpu().numpy()

    loss_dev, steps_dev = run(batches[:3])
    loss_host, steps_host = run([(x.cpu().numpy(), y.cpu().numpy()) for x, y in batches[:3]])
    assert np.isfinite(loss_dev) and np.all(np.isfinite(steps_dev))
    assert np.array_equal(steps_dev, steps_host) and loss_dev == loss_host

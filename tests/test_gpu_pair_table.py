"""GPU: the pair table's owner on its own (wikipedia/pair_table.py: PairTable) -- lazy creation, the growth rule through a
settle and a forced rehash, and the failure word -- filled through ops.cooccur_accumulate with W = 1 on 8 tokens in 2
documents.  The builders on top of it are held bit for bit against their restatements in test_gpu_cooccur.py,
test_gpu_dice.py and test_gpu_terms.py."""
import pytest
import torch

from esrecsys_amd import ops
from esrecsys_amd.wikipedia.pair_table import FAILURES, CooccurrenceError, PairTable

pytestmark = pytest.mark.gpu


def _entries(result):
    return [tuple(col) for col in zip(*(x.tolist() for x in result))]


def test_pair_table_grows_by_its_rule_and_fails_for_good(dev):
    """W = 1: position i adds 1 to (t[i], t[i - 1]) when t[i] > t[i - 1], inside its document.
    [1, 2, 3, 4] -> (2,1) (3,2) (4,3);  [9, 3, 4, 9] -> (4,3) again and (9,4); nothing for 3 < 9 or across the boundary."""
    tokens = torch.tensor([1, 2, 3, 4, 9, 3, 4, 9], dtype=torch.int32, device=dev)
    off = torch.tensor([0, 4, 8], dtype=torch.int64, device=dev)
    failures = dict(FAILURES)
    failures[2] = "a negative widget id"
    with torch.cuda.device(dev):
        t = PairTable(2, dev, failures, "widget table")
        assert t.tensor is None and (t.capacity, t.used, t.rehashes) == (2, 0, 0)
        assert _entries(t.finalize(10)) == [] and t.tensor is None       # nothing made for an empty result
        t.reserve(4)                                                     # made at the first launch's size
        assert t.capacity == 4 and t.rehashes == 0
        ops.cooccur_accumulate(t.tensor, t.capacity, tokens, off, 0, 4, 1)
        assert t.sync() == t.used == 3
        t.settle()                                                       # 3 of 4: doubled
        assert (t.capacity, t.rehashes, t.sync()) == (8, 1, 3)
        t.reserve(4)                                                     # 3 + 4 fit
        assert (t.capacity, t.rehashes) == (8, 1)
        ops.cooccur_accumulate(t.tensor, t.capacity, tokens, off, 4, 8, 1)
        assert t.sync() == 4
        t.settle()                                                       # 4 of 8: stays
        assert (t.capacity, t.rehashes) == (8, 1)
        expect = [(2, 1, 1.0), (3, 2, 1.0), (4, 3, 2.0), (9, 4, 1.0)]
        assert _entries(t.finalize(10)) == expect
        t.reserve(16)                                                    # forces a rehash
        assert (t.capacity, t.rehashes, t.sync()) == (32, 2, 4)
        index, other, count = t.finalize(10)
        assert _entries((index, other, count)) == expect and index.is_cuda and index.dtype == other.dtype == torch.int32
        assert count.dtype == torch.float32

        t.reserve(2)
        bad = torch.tensor([4, -2], dtype=torch.int32, device=dev)
        ops.cooccur_accumulate(t.tensor, t.capacity, bad, torch.tensor([0, 2], dtype=torch.int64, device=dev), 0, 2, 1)
        with pytest.raises(CooccurrenceError, match=r"^widget table failure \(bits 2\): a negative widget id$"):
            t.sync()
        for call in (t.check_usable, t.sync, t.settle, lambda: t.reserve(1), lambda: t.finalize(10)):
            with pytest.raises(CooccurrenceError, match="^this builder is unusable: a negative widget id$"):
                call()
        assert t.used == 4                                               # as of the last good sync

"""The class layout of the models trained by sampled SGD (esrecsys_amd/factorization.py): one trainer base under all five,
and SGNS -- which has no user table -- beside BPR, not below it."""
import numpy as np
import pytest


def test_one_trainer_base_and_sgns_beside_bpr():
    from esrecsys_amd import factorization as fz
    assert not issubclass(fz.SGNS, fz.BPR)
    for cls in (fz.BPR, fz.WARP, fz.HybridBPR, fz.FPMC, fz.SGNS):
        assert issubclass(cls, fz._SampledSGD), cls
    for cls in (fz.WARP, fz.HybridBPR, fz.FPMC):
        assert issubclass(cls, fz.BPR), cls
    for cls in (fz.FPMC, fz.SGNS):
        assert issubclass(cls, fz._Sequences), cls
    # what SGNS refuses is the base's (or its own), never an override of something BPR defines for it
    assert "_update" not in vars(fz._SampledSGD) and not hasattr(fz.SGNS, "_update")


@pytest.mark.gpu
def test_sgns_carries_no_seen_pairs():
    import torch
    from esrecsys_amd import factorization as fz
    doc = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int64)
    item = np.array([3, 5, 3, 7, 5, 7, 9, 3], np.int64)
    m = fz.SGNS(doc, item, window=2, negatives=2, rank=4, batch=8, device=torch.device("cuda", 0))
    for name in ("_row_ipos", "_row_upos", "_offsets_dev", "_key", "_user_offsets"):
        assert not hasattr(m, name), name
    assert m.n_events == 8 and m.nnz == 8 and m._failed.tolist() == [0]
    assert len(m.train_steps(2)) == 2 and m.step == 2
    for refused in (lambda: m.score([0], [3]), lambda: m.recommend([0]), lambda: m.auc()):
        with pytest.raises(TypeError, match="no user table"):
            refused()

"""Drop-in mirror of the reference's wikipedia/ hot path (models.py + train_cooccurence.py), of its two matrix makers
(make_cooccurrence.py, make_dice.py) and of the matrix's consumer (dump_dice.py: neighbours.py, with the item-kNN
recommender over the same table)."""
from . import make_dice  # noqa: F401
from . import neighbours  # noqa: F401

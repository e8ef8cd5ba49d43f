"""Drop-in mirror of the reference's wikipedia/ hot path (models.py + train_cooccurence.py) and of its two matrix makers
(make_cooccurrence.py, make_dice.py)."""
from . import make_dice  # noqa: F401

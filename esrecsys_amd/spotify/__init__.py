"""Drop-in mirror of the reference's ``spotify/`` package: SpotifyModel, train_step, eval_step."""
from .train_spotify import NegativeSampler, train_steps  # noqa: F401

"""Writes tests/golden/sgns_planted.json: the fp64 restatement's result on the planted two-community corpus
(tests/_sgns_ref.py planted_run) that tests/test_sgns_ref.py re-derives and tests/test_gpu_sgns.py takes its bar from.

    python tests/golden/make_sgns_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), os.path.join(HERE, "..", "..")]

import numpy as np  # noqa: E402

import _sgns_ref as sref  # noqa: E402

if __name__ == "__main__":
    share, losses = sref.planted_run(np.float64)
    out = {"settings": sref.PLANTED, "chance": sref.CHANCE, "own_share_at_5": share,
           "bar": sref.CHANCE + 0.5 * (share - sref.CHANCE), "first_loss": losses[0], "last_loss": losses[-1]}
    with open(os.path.join(HERE, "sgns_planted.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(out)

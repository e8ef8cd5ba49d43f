"""GPU: the models of esrecsys_amd/factorization.py train bit for bit what they trained before they were given one
base class (FPMC and SGNS: before the sampled-SGD family was given one sampler shell, one logistic and one trainer base).
tests/golden/make_factorization_golden.py trains small models (every rank layout, row-length class, optimiser and launch slicing) and digests every table, loss list and a few outputs with SHA-256; tests/golden/factorization_parent.json
holds those digests as written at the parent commit (stable between two runs there).  The models are functions of their
inputs and the seed, so equality is the assertion: a reordered generator draw or ops call shows as a different table.
(The digests of the two ALS models were written again when the pivot's square root in esr_als.hip became the correctly
rounded one, which tests/test_gpu_als_exact.py demands: last bits of every solved row moved; the other twelve models kept
theirs.)"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def maker():
    spec = importlib.util.spec_from_file_location("make_factorization_golden",
                                                  os.path.join(GOLDEN, "make_factorization_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "factorization_parent.json")) as f:
        return json.load(f)


FAMILIES = {"als": ("RatingsALS", "ImplicitALS"), "bpr": ("BPR",), "warp": ("WARP",), "hybrid": ("HybridBPR",),
            "fpmc": ("FPMC",), "sgns": ("SGNS",)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_models_are_the_parents_bit_for_bit(maker, parent, family):
    got = maker.compute(family)
    assert set(maker.FAMILIES) == set(FAMILIES)
    # both ways: every model of the fixture whose name starts with one of the family's classes is retrained, and no other
    assert set(got) == {name for name in parent if name.split(" ")[0] in FAMILIES[family]}, family
    for model, tables in got.items():
        assert model in parent, "%s is not in the fixture" % model
        want = [tuple(p) for p in parent[model]]
        assert [name for name, _ in tables] == [name for name, _ in want], model
        for (name, sha), (_, sha_want) in zip(tables, want):
            assert sha == sha_want, "%s: %s differs from the parent's (the first that does)" % (model, name)

"""CPU: what engine.py's block operations (reduce, tstat, quantile, quantiles,
outliers, argext, masked reduce, histogram, hits, fold, unfold; single, plan,
band and host forms) answer to a call that is wrong once, and which refusal wins
when it is wrong twice (engine_front_cases.py).  The inputs are CPU torch tensors
and NumPy arrays, so a device form that passes every check before ``_abi_dims``
answers its "device tensor expected"; test_gpu_engine_front.py goes on from
there.  golden/engine_front_errors.json was recorded by running engine.py as it
stood at 8090412, before the forms shared their helpers, not derived from it."""
from __future__ import annotations

import json
import os

import pytest

import engine_front_cases as cases

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "engine_front_errors.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as fh:
        return cases.unpack(json.load(fh))


@pytest.fixture(scope="module")
def got(pkg):
    import torch

    return cases.answers(pkg, torch, "cpu", gpu=False)


def test_table_is_whole(want, got):
    assert sorted(want) == sorted(got)
    assert len(want) > 2000
    fams = {k.split("/")[0] for k in want}
    assert fams == set(cases.FAMILIES)
    assert {k.split("/")[1] for k in want} == set(cases.FORMS)


def test_every_row_is_refused_or_reaches_the_device(want):
    for key, a in want.items():
        assert a[0] != "ok" and a[2], key


def test_classes_codes_and_messages(want, got):
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} rows differ, e.g. {sorted(wrong.items())[:5]}"

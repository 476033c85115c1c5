"""MI355X: the table of test_engine_front_errors.py with device tensors, which
reaches what a CPU tensor cannot: an out, mask or profile on the host, banks of
different shape or layout, out strides one too short, a band out that is not
dense, idx and val of different strides.  And one good call of every family and
form (again with a caller's out where one is taken): the results' dtypes, shapes
and strides, and every plan's keys and values.  Every call returns before a launch
or launches a 256-element window.  golden/engine_front_errors_gpu.json was
recorded on an MI355X by running engine.py as it stood at 8090412."""
from __future__ import annotations

import json
import os

import pytest

import engine_front_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "engine_front_errors_gpu.json")


# The one rewording since the recording: "all banks agree" is now stated once
# (engine._banks), so the two refusals that _band_args and band_hits worded apart
# read as the moments' and the fold's always did.  Still a ValueError, and the
# same rows; golden keeps what 8090412 answered.
_SAME = "all banks of a band must have the same "
REWORDED = {_SAME + "shape": _SAME + "shape and layout",
            _SAME + "layout": _SAME + "shape and layout"}


@pytest.fixture(scope="module")
def golden_tables():
    with open(GOLDEN) as fh:
        g = json.load(fh)
    errors = {k: [a[0], a[1], REWORDED.get(a[2], a[2])] if a[0] == "ValueError" else a
              for k, a in cases.unpack(g["errors"]).items()}
    return errors, cases.unpack(g["good"])


def test_classes_codes_and_messages(pkg, golden_tables):
    import torch

    want = golden_tables[0]
    got = cases.answers(pkg, torch, "cuda:0", gpu=True)
    torch.cuda.synchronize()
    assert sorted(want) == sorted(got) and len(want) > 3000
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} rows differ, e.g. {sorted(wrong.items())[:5]}"


def test_good_calls_and_plans(pkg, golden_tables):
    import torch

    want = golden_tables[1]
    got = json.loads(json.dumps(cases.good(pkg, torch, "cuda:0")))
    torch.cuda.synchronize()
    assert sorted(want) == sorted(got)
    assert all(a[0] == "ok" for a in want.values())
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} calls differ, e.g. {sorted(wrong.items())[:5]}"

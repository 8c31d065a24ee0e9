"""The bound kernels give the bits they gave before they shared their bodies (omc_bounds_dev.h).

tests/golden/bounds_parent_bits.json was recorded by tools/capture_bounds_bits.py with the library of the commit before
that change.  The bodies perform that commit's operations in its order, so every output is equal, not merely close: the
bounds and their standard errors as float.hex(), the counts, and SHA-256 of the bytes of Q^ and of the samples.  The cases
(tests/helpers/bounds_bits_case.py) reach all 18 kernels: the vanilla pair for put and call, the basket pair for d = 1 .. 8,
a partial Philox block, the refill, fitted and given policies, the float64 stopping rule."""
import json
import os

import pytest

from helpers import bounds_bits_case as bb

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bounds_parent_bits.json")) as f:
    RECORDED = json.load(f)


def test_the_cases_are_the_recorded_ones():
    assert {c["name"] for c in bb.cases()} == set(RECORDED) and len(RECORDED) == 10
    assert {c["d"] for c in bb.cases()} == set(range(9))  # 0: the vanilla entry


@pytest.mark.parametrize("case", bb.cases(), ids=lambda c: c["name"])
def test_bits_of_the_recorded_commit(ctx, case):
    got, want = bb.run(ctx, case), RECORDED[case["name"]]
    print(case["name"], got)
    assert got["n_exercised_lower"] > 0 and got["inner_path_steps"] > bb.N_OUTER * bb.N_INNER  # the case decides something
    for k in want:
        assert got[k] == want[k], (case["name"], k)
    assert set(got) == set(want)

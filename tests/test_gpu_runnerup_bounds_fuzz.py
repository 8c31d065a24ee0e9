"""A seeded sweep of omc_price_american_basket_bounds_runnerup against the numpy restatement on the device's own spots, as
tests/test_gpu_runnerup_bounds.py::test_device_equals_restatement does it for fixed shapes: d in 2 .. 8, both kinds, N in
1 .. 13 (partial Philox blocks, a single date), n_inner in {2, 64, 130, 200} (one pair, a full wave, the refill), a ragged
n_outer, fitted policies and given tables with n = 0 holes.  The cases come from helpers/runnerup_ref.fuzz_cases (checked
without a GPU in test_runnerup_bounds_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import numpy as np
import pytest

from helpers import basket_bounds_case as bc
from helpers import runnerup_ref as rr

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(12 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", rr.fuzz_cases(N_CASES), ids=lambda c: f"d{c['d']}-{c['kind']}-N{c['N']}-i{c['n_inner']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p, b = bc.fuzz_params(case)
    given = rr.given_table(ctx, p, b, case["holes"]) if case["policy"] == "given" else None
    dev = ctx.price_american_basket_bounds(p, b, policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"],
                                           n_inner=case["n_inner"], betas=given, want_q=True, want_samples=True,
                                           regressors=rr.REG)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    else:  # the fit, date by date, on the device's own fitting paths
        X, Y = rr.paths_xy(ctx, p, b)
        rr.check_fit(X, Y, float(p.K), p.r, p.T, bool(p.is_put), dev["betas"])
    rr.check_against_restatement(ctx, p, b, dev, case["n_lower"], case["n_outer"], case["n_inner"])

"""A seeded sweep of omc_price_american_basket_bounds against the numpy restatement on the device's own spots, as
tests/test_gpu_basket_bounds.py::test_device_equals_restatement does it for fixed shapes: d in 1 .. 8, the three kinds,
N in 1 .. 13 (partial Philox blocks, a single date), n_inner in {2, 64, 130, 200} (one pair, a full wave, the refill), a ragged
n_outer, fitted policies and given tables with n = 0 holes, the float64 fallback.  The cases come from
helpers/basket_bounds_case.fuzz_cases (checked without a GPU in test_basket_bounds_cases_cpu.py); OMC_FUZZ_SCALE scales
their number."""
import os

import numpy as np
import pytest

from helpers import basket_bounds_case as bc

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(12 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", bc.fuzz_cases(N_CASES), ids=lambda c: f"d{c['d']}-{c['kind']}-N{c['N']}-i{c['n_inner']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p, b = bc.fuzz_params(case)
    given = bc.fuzz_given_table(ctx, p, b, case["holes"]) if case["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        dev = ctx.price_american_basket_bounds(p, b, policy=case["policy"], n_lower=case["n_lower"],
                                               n_outer=case["n_outer"], n_inner=case["n_inner"], betas=given, want_q=True,
                                               want_samples=True)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    else:
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, b, case["policy"]))
    bc.check_against_restatement(ctx, p, b, dev, case["n_lower"], case["n_outer"], case["n_inner"])

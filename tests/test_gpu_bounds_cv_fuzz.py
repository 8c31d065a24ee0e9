"""A seeded sweep of the GBM price bounds with the Black-Scholes control variate (option "bounds_control_variate", DESIGN.md
section 26) against the numpy restatement on the device's own spots, as tests/test_gpu_bounds_cv.py::
test_device_equals_restatement does it for fixed shapes: N in 1 .. 13, every third case with a schedule k in 2 .. N + 3, n_inner
over every lane group, a ragged group and the refill, a ragged n_outer, put and call, fitted policies and given tables with
n = 0 holes, the float64 fallback on some cases.  The cases come from helpers/bounds_cv_ref.fuzz_cases (checked without a GPU
in test_bounds_cv_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import numpy as np
import pytest

from helpers import bounds_cv_ref as cv
from helpers import bounds_schedule_ref as bs

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", cv.fuzz_cases(N_CASES),
                         ids=lambda c: f"N{c['N']}-k{c['k']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p = bs.fuzz_params(case)
    k = case["k"]
    given = bs.given_table(ctx, p, case["holes"]) if case["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        kw = dict(policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"], n_inner=case["n_inner"], betas=given,
                  want_q=True, want_samples=True, exercise_every=k)
        dev = ctx.price_american_bounds(p, control_variate=True, **kw)
        plain = ctx.price_american_bounds(p, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    np.testing.assert_array_equal(dev["betas"], plain["betas"])
    assert dev["n_exercised_lower"] == plain["n_exercised_lower"] and dev["inner_path_steps"] == plain["inner_path_steps"]
    sp = bs.device_spots(ctx, p, k, case["n_lower"], case["n_outer"], case["n_inner"])
    dv = cv.check_against_restatement(p, dev, sp, k, case["n_lower"], case["n_outer"], case["n_inner"], cv.CV_TOL)
    print("fuzz " + ", ".join(f"{key} {v:.3e}" for key, v in dv.items()))

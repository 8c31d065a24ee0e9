"""A seeded sweep of the price bounds with an exercise schedule (option "bounds_exercise_every") against
the numpy restatement on the device's own spots, as tests/test_gpu_bounds_schedule.py::test_device_equals_restatement does it
for fixed shapes: N in 1 .. 13, k in 0 .. N + 3 (every date, a short first gap, dates inside a Philox block, gaps longer than
one, the expiry alone), n_inner in {2, 64, 130, 200} (one pair, a full wave, the refill), a ragged n_outer, GBM and both Heston
schemes, put and call, fitted policies and given tables with n = 0 holes, the float64 fallback on some cases.  The cases come
from helpers/bounds_schedule_ref.fuzz_cases (checked without a GPU in test_bounds_schedule_cpu.py); OMC_FUZZ_SCALE scales
their number."""
import os

import numpy as np
import pytest

from helpers import bounds_schedule_ref as bs

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", bs.fuzz_cases(N_CASES),
                         ids=lambda c: f"{c['model']}-N{c['N']}-k{c['k']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p = bs.fuzz_params(case)
    k = case["k"]
    given = bs.given_table(ctx, p, case["holes"]) if case["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        dev = bs.price(ctx, p, policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"], n_inner=case["n_inner"],
                       betas=given, want_q=True, want_samples=True, exercise_every=k)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], bs.mask(given, k))
    else:  # omc_lsm_poly's fits on the gathered matrix of the device's own fitting paths
        np.testing.assert_array_equal(dev["betas"], bs.fitted_table(ctx, p, case["policy"], k))
    sp = bs.device_spots(ctx, p, k, case["n_lower"], case["n_outer"], case["n_inner"])
    bs.check_against_restatement(p, dev, sp, k, case["n_lower"], case["n_outer"], case["n_inner"])
    assert dev["inner_path_steps"] <= bs.max_inner_steps(case["N"], k, case["n_outer"], case["n_inner"])

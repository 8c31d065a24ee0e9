"""A seeded sweep of omc_price_american_bounds_heston against the numpy restatement on the device's own spots, as
tests/test_gpu_heston_bounds.py::test_device_equals_restatement does it for fixed shapes: N in 1 .. 13 (half-used Philox
blocks, partly used draws, a single date), n_inner in {2, 64, 130, 200} (one pair, a full wave, the refill), a ragged n_outer,
schemes 0 and 1, put and call, fitted policies and given tables with n = 0 holes, the float64 fallback on some cases, random
Heston parameters with every third case violating Feller.  The cases come from helpers/heston_bounds_case.fuzz_cases
(checked without a GPU in test_heston_bounds_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import numpy as np
import pytest

from helpers import heston_bounds_case as hc

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", hc.fuzz_cases(N_CASES),
                         ids=lambda c: f"s{c['scheme']}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p = hc.fuzz_params(case)
    given = hc.given_table(ctx, p, case["holes"]) if case["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        dev = ctx.price_american_bounds_heston(p, policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"],
                                               n_inner=case["n_inner"], betas=given, want_q=True, want_samples=True)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    else:  # omc_lsm_poly's fits on the device's own fitting paths
        np.testing.assert_array_equal(dev["betas"], hc.fitted_table(ctx, p, case["policy"]))
    sp = hc.device_spots(ctx, p, case["n_lower"], case["n_outer"], case["n_inner"])
    if not case["feller"] and case["scheme"] == 1 and case["N"] > 2:
        print("lowest outer variance state", float(sp["Vo"].min()))
    hc.check_against_restatement(p, dev, sp, case["n_lower"], case["n_outer"], case["n_inner"])

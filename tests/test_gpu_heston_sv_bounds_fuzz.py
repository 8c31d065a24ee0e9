"""A seeded sweep of omc_price_american_bounds_heston with the policy on the spot and the variance state against the numpy
restatement on the device's own states, as tests/test_gpu_heston_sv_bounds.py::test_device_equals_restatement does it for
fixed shapes: N in 1 .. 13 (partial Philox blocks, a single date), n_inner in {2, 64, 130, 200} (one pair, a full wave,
the refill), a ragged n_outer, both schemes, put and call, fitted policies and given tables with n = 0 holes, every third
case violating Feller (scheme 1 there: negative variance states).  The cases come from helpers/heston_sv_ref.fuzz_cases
(checked without a GPU in test_heston_sv_bounds_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import numpy as np
import pytest

from helpers import heston_bounds_case as hc
from helpers import heston_sv_ref as sv

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", sv.fuzz_cases(N_CASES),
                         ids=lambda c: f"N{c['N']}-i{c['n_inner']}-s{c['scheme']}-{c['policy']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p = hc.fuzz_params(case)
    given = sv.given_table(ctx, p, case["holes"]) if case["policy"] == "given" else None
    dev = ctx.price_american_bounds_heston(p, policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"],
                                           n_inner=case["n_inner"], betas=given, want_q=True, want_samples=True,
                                           regressors=sv.REG)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    else:  # the fit, date by date, on the device's own fitting paths
        sv.check_fit(*sv.fitting_paths(ctx, p), float(p.K), p.r, p.T, bool(p.is_put), dev["betas"], sv.vbar_of(p))
    st = sv.device_states(ctx, p, case["n_lower"], case["n_outer"], case["n_inner"])
    sv.check_against_restatement(p, dev, st, case["n_lower"], case["n_outer"], case["n_inner"])
    if not case["feller"] and case["scheme"] == 1 and case["N"] > 4:
        assert st["Yo"].min() < 0.0  # inner items that start at a negative variance state

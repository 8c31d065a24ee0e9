"""Seeded fuzz of the Asian bounds (kind OMC_BASKET_ASIAN_ARITHMETIC of omc_price_american_basket_bounds and, with
regressors "index+spot", omc_price_american_basket_bounds_runnerup) against the numpy restatement of
tests/helpers/asian_ref.py on the device's own spots: random asset counts, correlations, weights, yields, dates (partial
Philox blocks, one date), ragged outer counts, inner counts below and above a wave (the refill), put and call, fitted and
given policies with n = 0 holes, the two regressor sets alternating.  OMC_FUZZ_SCALE scales the number of cases."""
import os

import numpy as np
import pytest

from helpers import asian_ref as ar
from helpers import basket_bounds_case as bc
from helpers import runnerup_ref as rr

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(6 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


def test_the_cases_cover_what_they_are_for():
    cases = ar.fuzz_cases(6)
    assert {c["regressors"] for c in cases} == {"index", ar.REG} and {c["policy"] for c in cases} == {"textbook", "given"}
    assert any(c["refill"] for c in cases) and any(not c["refill"] for c in cases)
    assert len({c["d"] for c in cases}) == 6 and any(c["N"] % 4 for c in cases)


@pytest.mark.parametrize("case", ar.fuzz_cases(N_CASES),
                         ids=lambda c: f"d{c['d']}-N{c['N']}-i{c['n_inner']}-{c['regressors']}-{c['policy']}")
def test_fuzz_case_equals_restatement(ctx, case):
    p, b = bc.fuzz_params(case)
    reg = case["regressors"]
    given = None
    if case["policy"] == "given":
        given = (ar.given_table4 if reg == "index" else ar.given_table8)(ctx, p, b, case["holes"])
    dev = ctx.price_american_basket_bounds(p, b, policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"],
                                           n_inner=case["n_inner"], betas=given, want_q=True, want_samples=True,
                                           regressors=reg)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    elif reg == "index":
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, b, "textbook"))
    else:  # the fit, date by date, on the device's own fitting paths
        _, _, X, B, _ = ar.paths(ctx, p, b)
        rr.check_fit(X, B, float(p.K), p.r, p.T, bool(p.is_put), dev["betas"])
    ar.check_against_restatement(ctx, p, b, dev, case["n_lower"], case["n_outer"], case["n_inner"], regressors=reg)

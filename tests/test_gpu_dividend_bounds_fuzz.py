"""A seeded sweep of omc_price_american_bounds_div against the numpy restatements on the device's own spots, as
tests/test_gpu_dividend_bounds.py does it for fixed shapes: random schedules of 0 .. 5 cash and proportional dividends, N in
1 .. 13, n_inner in {2, 64, 130, 200} (one pair, a full wave, the refill), a ragged n_outer, the three models and the four
policies cycled (given tables with n = 0 holes), put and call, a dividend yield on some, the float64 fallback on some, every
third case with an exercise schedule and every third with the payoff check.  The cases come from
helpers/dividend_bounds_case.fuzz_cases (checked without a GPU in test_dividend_bounds_cpu.py); OMC_FUZZ_SCALE scales their
number."""
import os

import numpy as np
import pytest

from helpers import bounds_check_ref as bk
from helpers import bounds_schedule_ref as bs
from helpers import dividend_bounds_case as dc

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


def _id(c):
    what = f"-k{c['every']}" if c["every"] else "-check" if c["check"] else ""
    return f"{c['model']}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}-d{len(c['divs'])}{what}"


@pytest.mark.parametrize("case", dc.fuzz_cases(N_CASES), ids=_id)
def test_fuzz_case_equals_restatement(ctx, case):
    p, divs, q, k = dc.case_params(case), dc.dividends_of(case), case["q"], case["every"]
    N, K, is_put = case["N"], case["K"], case["is_put"]
    given = dc.given_table(ctx, p, q, divs, case["holes"]) if case["policy"] == "given" else None
    kw = dict(policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"], n_inner=case["n_inner"], betas=given,
              want_q=True, want_samples=True)
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        dev = ctx.price_american_bounds_div(p, q, divs, exercise_every=k, **kw)
        got = ctx.price_american_bounds_div(p, q, divs, suboptimality_check="payoff", **kw) if case["check"] else None
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], bs.mask(given, k))
    else:  # omc_lsm_poly's fits on the device's own fitting paths
        np.testing.assert_array_equal(dev["betas"], dc.fitted_table(ctx, p, q, divs, case["policy"], k))
    ts = bs.schedule(N, k)[:-1] if k >= 2 else None
    sp = dc.device_spots(ctx, p, q, divs, case["n_lower"], case["n_outer"], case["n_inner"], ts=ts)
    if k >= 2:
        bs.check_against_restatement(p, dev, sp, k, case["n_lower"], case["n_outer"], case["n_inner"])
    else:
        dc.check_against_restatement(p, dev, sp, case["n_lower"], case["n_outer"], case["n_inner"])
    if got is not None:
        st = bk.item_steps(sp["So"], sp["inner"], range(case["n_outer"]), K, p.r, p.T, is_put, dev["betas"])
        assert st["ties"] == 0
        kp = bk.check_against_dense(p, dev, got, 1, sp["So"], None, st["steps"])
        print(f"items kept {kp.mean():.3f}, upper {got['upper']:.6f} (dense {dev['upper']:.6f})")

"""A seeded sweep of omc_price_american_div_greeks against the numpy restatement on the device's own matrices and normals,
as tests/test_gpu_dividend_greeks.py does it for fixed shapes and with its tolerances: random schedules of 0 .. 5 cash and
proportional dividends, N in 2 .. 13, a ragged n_paths, GBM and Heston schemes 0, 1 and 3 cycled, put and call, a dividend
yield on every other case, three bump sizes.  The cases come from helpers/dividend_greeks_case.fuzz_cases (checked without a
GPU in test_dividend_greeks_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import pytest

from helpers import dividend_bounds_case as dc
from helpers import dividend_greeks_case as gc
from test_gpu_dividend_greeks import compare

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(24 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


def _id(c):
    return f"{c['model']}-N{c['N']}-M{c['M']}-{'put' if c['is_put'] else 'call'}-d{len(c['divs'])}-h{c['h']}"


CASES = gc.fuzz_cases(N_CASES)


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_fuzz_case_against_the_restatement(ctx, c):
    p = gc.make_params(c["model"], is_put=c["is_put"], S0=c["S0"], N=c["N"], M=c["M"], seed=c["seed"], stream=c["stream"],
                       sigma=0.25)
    divs = dc.dividends_at(c["divs"], 1.0, c["N"])
    out, ref, _, res = compare(ctx, p, c["q"], divs, c["h"], label="fuzz-" + _id(c))
    base = res[0]
    if base["folded"] == 0:  # (a yield-only pricing may run folded: its fits come from other sums)
        assert (out["n_exercised"], out["n_zero"], out["sum_nitm"]) == (base["n_exercised"], base["n_zero"], base["sum_nitm"])

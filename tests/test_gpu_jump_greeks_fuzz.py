"""A seeded sweep of omc_price_american_jump_greeks against the numpy restatement on the device's own matrices and
normals, as tests/test_gpu_jump_greeks.py does it for its grid and with its tolerances: ragged pair counts up to 1200, N
in 1 .. 13, random jump laws and intensities, random sigma, r, T and S0, GBM and Heston schemes 0, 1 and 3 cycled, put and
call, a dividend yield on every other case, three bump sizes.  The cases come from helpers/jump_greeks_case.fuzz_cases
(checked without a GPU in test_jump_greeks_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import pytest

from helpers import jump_greeks_case as gc
from test_gpu_jump_greeks import SUM, compare

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


def _id(c):
    return f"{c['model']}-N{c['N']}-P{c['pairs']}-{'put' if c['is_put'] else 'call'}-x{c['x']:.3f}-h{c['h']}"


CASES = gc.fuzz_cases(N_CASES)


@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_fuzz_case_against_the_restatement(ctx, c):
    p = gc.case_params(c)
    out, ref, _, res = compare(ctx, p, gc.jump_of(c), c["q"], c["h"], label="fuzz-" + _id(c))
    base = res[0]
    assert (out["n_exercised"], out["n_zero"], out["sum_nitm"]) == (base["n_exercised"], base["n_zero"], base["sum_nitm"])
    assert abs(out["price"] - base["price"]) <= SUM * abs(base["price"])

"""A seeded sweep of omc_price_american_chain_bounds against every entry's own single call on the device, as
tests/test_gpu_chain_bounds.py does it for fixed shapes: GBM and both Heston schemes, N in 1 .. 13,
n_inner of 2, 64, 128 (exact) and 130, 512 (refills: the measured order-of-summation bound), a ragged n_outer, 1 .. cap + 2
entries of mixed sides with strikes from deep in to far out of the money, every policy with given tables of every kind, the
float64 fallback on some cases.  The cases come from helpers/chain_bounds_case.fuzz_cases (checked without a GPU in
tests/test_chain_bounds_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import pytest

from helpers import chain_bounds_case as cc

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(10 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", cc.fuzz_cases(N_CASES), ids=cc.case_id)
def test_fuzz_case_against_the_single_calls(ctx, case):
    outs, info = cc.run_chain(ctx, case)
    assert len(outs) == len(case["strikes"])
    for e, got in enumerate(outs):
        cc.compare(case, got, cc.run_single(ctx, case, e), 4.0 * cc.MEASURED_UPPER_REL, 4.0 * cc.MEASURED_Q_REL)
    cc.check_steps(outs, info)

"""A seeded sweep of omc_price_american_bounds_barrier against the numpy restatement on the device's own REAL spots, as
tests/test_gpu_barrier_bounds.py does it for fixed shapes: the four kinds cycled, a barrier 2 .. 10 % away from a random spot,
N in 1 .. 13, n_inner in {2, 64, 130, 200} (one pair, a full wave, the refill), a ragged n_outer, the three models and the
four policies cycled (given tables with n = 0 holes), put and call, the float64 fallback on some, every third case with an
exercise schedule and every third with the payoff check.  The cases come from helpers/barrier_bounds_case.fuzz_cases (checked
without a GPU in test_barrier_bounds_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import numpy as np
import pytest

from helpers import barrier_bounds_case as bc
from helpers import barrier_bounds_ref as bbr
from helpers import bounds_schedule_ref as bs

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


def _id(c):
    what = f"-k{c['every']}" if c["every"] else "-check" if c["check"] else ""
    return f"{c['model']}-{c['kind']}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}{what}"


@pytest.mark.parametrize("case", bc.fuzz_cases(N_CASES), ids=_id)
def test_fuzz_case_equals_restatement(ctx, case):
    p, kind, H, k, check = bc.case_params(case), case["kind"], case["H"], case["every"], case["check"]
    N = case["N"]
    sizes = (case["n_lower"], case["n_outer"], case["n_inner"])
    given = bc.given_table(ctx, p, case["holes"]) if case["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        dev = ctx.price_barrier_bounds(p, kind, H, policy=case["policy"], n_lower=sizes[0], n_outer=sizes[1], n_inner=sizes[2],
                                       betas=given, want_q=True, want_samples=True, exercise_every=k,
                                       suboptimality_check=check)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], bs.mask(given, k))
    else:  # omc_lsm_poly's fits on omc_price_barrier's encoded matrix
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, kind, H, case["policy"], k))
    ts = bs.schedule(N, k)[:-1] if k >= 2 else None
    sp = bc.device_spots(ctx, p, *sizes, ts=ts)
    lo, up = bbr.check_against_restatement(p, dev, sp, kind, H, k, check, *sizes)
    dead = bbr.dead_items(up["hit"], N, kind).T
    assert np.all(dev["q"][dead] == 0.0)
    assert dev["upper"] >= dev["lower"] - 3.0 * (dev["se_lower"] + dev["se_upper"])
    print(f"hit {np.count_nonzero(up['hit']) / up['hit'].size:.2f}, items kept {up['keep'].mean():.3f}, bounds "
          f"[{dev['lower']:.6f}, {dev['upper']:.6f}], steps {dev['inner_path_steps']}")

"""A seeded sweep of the price bounds with sub-optimality checking (option "bounds_suboptimality") against
the dense call and the numpy restatement on the device's own spots, as tests/test_gpu_bounds_check.py::
test_checked_call_against_the_dense_call does it for fixed shapes: every model that takes a check (GBM plain and controlled,
a two-asset basket, the arithmetic Asian index, Heston full truncation), the European check on the GBM ones, N in 1 .. 13,
n_inner over every lane group, a ragged group and the refill, a ragged n_outer, put and call, fitted policies and given tables
with n = 0 holes, the float64 fallback on some cases.  The cases come from helpers/bounds_check_ref.fuzz_cases (checked without
a GPU in test_bounds_check_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import pytest

from helpers import bounds_check_ref as bk

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


@pytest.mark.parametrize("case", bk.fuzz_cases(N_CASES),
                         ids=lambda c: f"{c['model']}-m{c['mode']}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{c['policy']}")
def test_fuzz_case_against_the_dense_call(ctx, case):
    model, mode, N = case["model"], case["mode"], case["N"]
    p, b = bk.params_of(model, is_put=case["is_put"], S0=case["S0"], K=case["K"], r=case["r"], sigma=case["sigma"], T=case["T"],
                        N=N, M=case["M"], seed=case["seed"], stream=case["stream"])
    given = bk.given_table(ctx, model, p, b, case["holes"]) if case["policy"] == "given" else None
    kw = dict(policy=case["policy"], n_lower=case["n_lower"], n_outer=case["n_outer"], n_inner=case["n_inner"], betas=given,
              want_q=True, want_samples=True)
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        dense = bk.call(ctx, model, p, b, 0, **kw)
        got = bk.call(ctx, model, p, b, mode, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    sp = bk.device_spots(ctx, model, p, b, 2, case["n_outer"], case["n_inner"])
    try:
        st = bk.item_steps(sp["So"], sp["inner"], range(case["n_outer"]), case["K"], case["r"], case["T"], case["is_put"],
                           dense["betas"])
    finally:
        sp["free"]()
    assert st["ties"] == 0
    kp = bk.check_against_dense(p, dense, got, mode, sp["So"], case["sigma"], st["steps"])
    print(f"fuzz {model} mode {mode}: items kept {kp.mean():.3f}, inner steps kept "
          f"{got['inner_path_steps'] / max(dense['inner_path_steps'], 1):.3f}")
    assert ctx._bounds_check == 0

"""A seeded sweep of the Heston QE generator (scheme 3) against the float64 restatement on the device's own normals, as
tests/test_gpu_heston_qe.py::test_device_against_the_restatement_per_spot does it for fixed shapes: random laws (every third
violates Feller, so its waves mix the two branches), 1 .. 70 steps, ragged pair counts (every store width), pair offsets.
The same exclusion rule and cap; the bound is the project's 5e-5 up to 64 steps and grows with the step count beyond it
(rounding errors add up at most linearly in the steps: 5e-5 n / 64 for n > 64).  The cases come from
helpers/heston_qe_ref.fuzz_cases (checked without a GPU in tests/test_heston_qe_cpu.py); OMC_FUZZ_SCALE scales their number."""
import os

import numpy as np
import pytest

from helpers import heston_qe_ref as qe

pytestmark = pytest.mark.gpu

N_CASES = max(1, int(round(8 * float(os.environ.get("OMC_FUZZ_SCALE", "1")))))


def _host(a):
    h = a.to_host()
    a.free()
    return h


@pytest.mark.parametrize("case", qe.fuzz_cases(N_CASES), ids=lambda c: f"N{c['N']}-p{c['pairs']}-xi{c['xi']:.2f}")
def test_fuzz_case_equals_restatement(ctx, case):
    c = case
    H, N = c["pairs"], c["N"]
    hp = [c[k] for k in ("v0", "kappa", "theta", "xi", "rho")]
    S = _host(ctx.heston_paths(2 * H, N, c["S0"], c["r"], c["T"], *hp, c["seed"], c["stream"], c["pair_offset"], 3))
    Sd, Vd = ctx.heston_paths_sv(2 * H, N, c["S0"], c["r"], c["T"], *hp, c["seed"], c["stream"], c["pair_offset"], 3)
    S2, V = _host(Sd), _host(Vd)
    assert np.array_equal(S2.view(np.uint32), S.view(np.uint32)) and V.min() >= 0.0 and np.isfinite(S).all()
    z1, z2 = qe.pair_view(_host(ctx.gbm_normals(H, 2 * N, c["seed"], c["stream"], c["pair_offset"])))
    ref = qe.paths(z1, z2, c["S0"], c["v0"], c["r"], c["T"], c["kappa"], c["theta"], c["xi"], c["rho"])
    got = qe.compare(S, ref, qe.RTOL * max(1.0, N / 64.0))
    print(f"worst {got['worst']:.3e} left out {got['share']:.4f} exponential {ref['expo'].mean():.3f}")
    assert got["share"] <= qe.MAX_SHARE, got

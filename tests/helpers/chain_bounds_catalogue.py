"""The fixed cases of the chain price-bound tests (tests/test_gpu_chain_bounds.py).  TEST
INFRASTRUCTURE ONLY.  Shapes: n_steps 5, 8 (the four-step block ends on a date) and 9 (a block tail of one step, the odd
Heston half-block), n_outer 64 .. 256, n_lower 4096, n_paths 8192; n_inner 2, 64 and 128 where no lane is refilled (the
exact cases) and 130 and 512 where lanes are (the tolerance cases).  Chains of 1, 2, 3, the cap and the cap + 1 (two groups)
entries, mixed sides, a deep in-the-money strike (stops at the first date) beside a far out-of-the-money one (never stops
before N), given tables with an all-zero one among them, and the float64 rule on irregular dates."""
from __future__ import annotations

from helpers.chain_bounds_case import CAP, make_case

HESTON_FT = dict(model="heston", scheme=1, xi=1.0)  # full truncation where Feller fails: the variance goes below zero

_LADDER = [80.0, 90.0, 95.0, 100.0, 105.0, 110.0, 120.0, 130.0, 70.0]
_SIDES = [True, False, True, True, False, True, False, True, False]


def _chain(E):
    return dict(strikes=_LADDER[:E], puts=_SIDES[:E])


# n_inner <= 128: every output carries the bits of the entry's own single call
EXACT_CASES = {
    "gbm-E1-N5-i2": make_case(N=5, n_inner=2, n_outer=64, **_chain(1)),
    "gbm-E2-N8-i64": make_case(N=8, n_inner=64, n_outer=64, **_chain(2)),
    "gbm-E3-N9-i128": make_case(N=9, n_inner=128, n_outer=66, **_chain(3)),
    "gbm-cap-N9-i128-two_pass": make_case(N=9, n_inner=128, n_outer=64, policy="two_pass", **_chain(CAP)),
    "gbm-cap+1-N8-i64-reference": make_case(N=8, n_inner=64, n_outer=64, policy="reference", **_chain(CAP + 1)),
    # deep in the money (stops at date 1) beside far out of the money (never before N): lanes stay live for some entries
    "gbm-deep-far-N9-i128": make_case(N=9, n_inner=128, n_outer=64, strikes=[300.0, 20.0, 100.0], puts=True),
    "gbm-given-N8-i64": make_case(N=8, n_inner=64, n_outer=64, policy="given", given=["zero", "flat", "holes", "curve"],
                                  **_chain(4)),
    "gbm-irregular-N9-i128": make_case(N=9, n_inner=128, n_outer=64, irr_every=2, **_chain(3)),
    "heston-E2-N9-i64": make_case(model="heston", N=9, n_inner=64, n_outer=64, **_chain(2)),
    "heston-ft-cap-N8-i128": make_case(N=8, n_inner=128, n_outer=64, **HESTON_FT, **_chain(CAP)),
    "heston-ft-deep-far-irregular-N5-i2": make_case(N=5, n_inner=2, n_outer=256, irr_every=3, strikes=[300.0, 20.0],
                                                    puts=[True, True], **HESTON_FT),
    "heston-given-cap+1-N9-i128": make_case(model="heston", N=9, n_inner=128, n_outer=64, policy="given",
                                            given=["zero", "curve", "flat"] * 3, **_chain(CAP + 1)),
}

# n_inner > 128: lanes are refilled; q, samples and upper within the measured order-of-summation deviation
TOLERANCE_CASES = {
    "gbm-E3-N9-i130": make_case(N=9, n_inner=130, n_outer=64, **_chain(3)),
    "gbm-cap-N8-i512": make_case(N=8, n_inner=512, n_outer=64, **_chain(CAP)),
    "gbm-deep-far-N9-i512": make_case(N=9, n_inner=512, n_outer=64, strikes=[300.0, 20.0, 100.0], puts=True),
    "gbm-E1-N5-i130": make_case(N=5, n_inner=130, n_outer=128, **_chain(1)),
    "gbm-cap+1-irregular-N9-i130": make_case(N=9, n_inner=130, n_outer=64, irr_every=2, **_chain(CAP + 1)),
    "heston-E2-N9-i512": make_case(model="heston", N=9, n_inner=512, n_outer=64, **_chain(2)),
    "heston-ft-cap-N8-i130": make_case(N=8, n_inner=130, n_outer=64, **HESTON_FT, **_chain(CAP)),
}

# two identical entries give identical outputs; the simulated steps are then the entry's own count
TWIN_CASES = {
    "gbm-twins-N8-i64": make_case(N=8, n_inner=64, n_outer=64, strikes=[105.0, 105.0], puts=True),
    "gbm-twins-N9-i512": make_case(N=9, n_inner=512, n_outer=64, strikes=[95.0, 95.0, 95.0], puts=False),
    "heston-twins-N9-i130": make_case(model="heston", N=9, n_inner=130, n_outer=64, strikes=[100.0, 100.0], puts=True),
}

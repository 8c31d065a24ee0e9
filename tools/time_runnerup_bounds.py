"""HIP-event cost of omc_price_american_basket_bounds_runnerup on the max-call benchmark of Broadie-Glasserman /
Andersen-Broadie (best-of call, S0 = K = 100, r = 5 %, yield 10 %, sigma = 20 %, rho = 0, T = 3, nine dates; textbook policy
fitted on 100,000 paths; default sizes n_lower 1M, n_outer 8192, n_inner 1024) for d = 2, 4, 8 assets.  Three calls alternate
with every repetition in the same process:
  index      omc_price_american_basket_bounds, the policy on the index alone (float32 exercise tables);
  runnerup   the new entry point with its own fitted policy;
  same_rule  the new entry point GIVEN the index policy's coefficients (c3 = c4 = c5 = 0): the new kernels on exactly the
             index policy's inner paths -- the same decisions, the same path-steps --, so its upper phase against `index` is
             what the runner-up pass and the float64 polynomial cost per step, and `runnerup` against it is what the other
             policy's path lengths change.
Prints one JSON line per d: median event times of fit / lower / upper / total, inner path-steps, path- and asset-steps per
second of the upper phase, the ratios, the bounds.  usage: time_runnerup_bounds.py [reps] [N] [d ...]"""
import json
import os
import statistics as st
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
N = int(sys.argv[2]) if len(sys.argv) > 2 else 9
ds = [int(v) for v in sys.argv[3:]] or [2, 4, 8]
ctx = _ffi.default_context(0)
p = _ffi.make_params(semantics="two_pass", is_put=False, n_paths=100_000, n_steps=N, S0=100.0, K=100.0, r=0.05, sigma=0.2,
                     T=3.0, seed=42)
KEYS = ("ms_fit", "ms_lower", "ms_upper", "ms_total")
REG = "index+runner-up"


def summary(rs, d):
    r0 = rs[0]
    ms = {k[3:]: st.median(r[k] for r in rs) for k in KEYS}
    rate = r0["inner_path_steps"] / (ms["upper"] * 1e-3)
    return dict(ms=ms, inner_path_steps=r0["inner_path_steps"], inner_path_steps_per_s=rate, inner_asset_steps_per_s=d * rate,
                lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"],
                n_exercised_lower=r0["n_exercised_lower"])


def run(d):
    b = _ffi.make_basket([100.0] * d, [0.2] * d, [0.1] * d, [1.0] * d, None, "best-of")
    first = ctx.price_american_basket_bounds(p, b)  # warm-up: code objects, workspaces -- and the index policy's table
    b8 = np.zeros((N + 1, 8))
    b8[:, :3], b8[:, 6] = first["betas"][:, :3], first["betas"][:, 3]
    calls = dict(index=lambda: ctx.price_american_basket_bounds(p, b),
                 runnerup=lambda: ctx.price_american_basket_bounds(p, b, regressors=REG),
                 same_rule=lambda: ctx.price_american_basket_bounds(p, b, policy="given", betas=b8, regressors=REG))
    for f in calls.values():
        f()
    rs = {k: [] for k in calls}
    for _ in range(reps):  # alternated: all see the same clocks and the same neighbours
        for k, f in calls.items():
            rs[k].append(f())
    out = {k: summary(v, d) for k, v in rs.items()}
    ix, ru, sr = out["index"], out["runnerup"], out["same_rule"]
    return dict(d=d, N=N, reps=reps, n_lower=first["n_lower"], n_outer=first["n_outer"], n_inner=first["n_inner"], **out,
                same_rule_has_the_index_bits=bool((sr["lower"], sr["upper"], sr["inner_path_steps"]) ==
                                                  (ix["lower"], ix["upper"], ix["inner_path_steps"])),
                ratio_total=ru["ms"]["total"] / ix["ms"]["total"], ratio_upper=ru["ms"]["upper"] / ix["ms"]["upper"],
                ratio_upper_same_rule=sr["ms"]["upper"] / ix["ms"]["upper"],
                ratio_inner_path_steps=ru["inner_path_steps"] / ix["inner_path_steps"],
                ratio_lower_phase=ru["ms"]["lower"] / ix["ms"]["lower"])


for d in ds:
    print(json.dumps(run(d)), flush=True)

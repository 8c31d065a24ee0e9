"""HIP-event cost of omc_price_american_bounds_heston with the policy on the spot and the variance state (DESIGN.md section
21) on section 20.4's call: the ATM put (S0 = K = 100, r = 0.05, T = 1, N = 50; v0 = theta = 0.04, kappa = 2, xi = 0.3,
rho = -0.7; textbook policy fitted on 100,000 paths; default sizes n_lower 1M, n_outer 8192, n_inner 1024), schemes reference
and full_truncation.  Three calls alternate with every repetition in the same process:
  spot       regressors "spot": the policy on the spot alone (float32 exercise tables) -- the yardstick;
  variance   regressors "spot+variance" with its own fitted policy;
  same_rule  the new kernels GIVEN the spot policy's coefficients (c3 = c4 = c5 = 0): exactly the spot policy's decisions and
             inner paths, bits checked in the run, so its upper phase against `spot` is what the float64 polynomial in the
             place of the tables costs per step, and `variance` against it is what the other policy's path lengths change.
Prints one JSON line per scheme: median event times of fit / lower / upper / total, inner path-steps, path-steps per second
of the upper phase, the ratios, the two brackets.  usage: time_heston_sv_bounds.py [reps] [N] [extra: feller_off]"""
import json
import os
import statistics as st
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
if "feller_off" in sys.argv[3:]:  # the high vol-of-vol set of the tests: 2 kappa theta < xi^2
    HP = dict(v0=0.04, kappa=1.0, theta=0.09, xi=0.9, rho=-0.7)
ctx = _ffi.default_context(0)
KEYS = ("ms_fit", "ms_lower", "ms_upper", "ms_total")
REG = "spot+variance"


def summary(rs):
    r0 = rs[0]
    ms = {k[3:]: st.median(r[k] for r in rs) for k in KEYS}
    gap = r0["upper"] - r0["lower"]
    return dict(ms=ms, inner_path_steps=r0["inner_path_steps"], inner_path_steps_per_s=r0["inner_path_steps"] / (ms["upper"] * 1e-3),
                lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"], gap=gap,
                gap_rel=gap / r0["lower"], n_exercised_lower=r0["n_exercised_lower"])


def run(scheme):
    p = _ffi.make_params(model="heston", heston_scheme=scheme, is_put=True, semantics="two_pass", n_paths=100_000, n_steps=N,
                         S0=100.0, K=100.0, r=0.05, sigma=0.0, T=1.0, seed=42, **HP)
    first = ctx.price_american_bounds_heston(p)  # warm-up: code objects, workspaces -- and the spot policy's table
    b8 = np.zeros((N + 1, 8))
    b8[:, :3], b8[:, 6] = first["betas"][:, :3], first["betas"][:, 3]
    calls = dict(spot=lambda: ctx.price_american_bounds_heston(p),
                 variance=lambda: ctx.price_american_bounds_heston(p, regressors=REG),
                 same_rule=lambda: ctx.price_american_bounds_heston(p, policy="given", betas=b8, regressors=REG))
    for f in calls.values():
        f()
    rs = {k: [] for k in calls}
    for _ in range(reps):  # alternated: all see the same clocks and the same neighbours
        for k, f in calls.items():
            rs[k].append(f())
    out = {k: summary(v) for k, v in rs.items()}
    sp, va, sr = out["spot"], out["variance"], out["same_rule"]
    same = all(sr[k] == sp[k] for k in ("lower", "se_lower", "upper", "se_upper", "inner_path_steps", "n_exercised_lower"))
    return dict(N=N, reps=reps, scheme=scheme, heston=HP, n_lower=first["n_lower"], n_outer=first["n_outer"],
                n_inner=first["n_inner"], **out, same_rule_has_the_spot_bits=bool(same),
                ratio_total=va["ms"]["total"] / sp["ms"]["total"], ratio_upper=va["ms"]["upper"] / sp["ms"]["upper"],
                ratio_upper_same_rule=sr["ms"]["upper"] / sp["ms"]["upper"],
                ratio_lower_phase=va["ms"]["lower"] / sp["ms"]["lower"], ratio_fit=va["ms"]["fit"] / sp["ms"]["fit"],
                ratio_inner_path_steps=va["inner_path_steps"] / sp["inner_path_steps"],
                lower_gain=va["lower"] - sp["lower"], lower_gain_se=float(np.hypot(va["se_lower"], sp["se_lower"])),
                upper_change=va["upper"] - sp["upper"])


for scheme in ("reference", "full_truncation"):
    print(json.dumps(run(scheme)), flush=True)

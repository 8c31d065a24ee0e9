"""HIP-event cost of omc_price_american_basket_bounds on the max-call benchmark of Broadie-Glasserman / Andersen-Broadie
(best-of call, S0 = K = 100, r = 5 %, yield 10 %, sigma = 20 %, rho = 0, T = 3, nine dates; textbook policy fitted on
100,000 paths; default sizes n_lower 1M, n_outer 8192, n_inner 1024) for d = 1, 2, 4, 8 assets, and, alternated with every
repetition in the same process, the single-asset omc_price_american_bounds at the same N and sizes (S0 = K = 100,
sigma = 20 %, no yield, call).  Prints one JSON line per d: median event times of fit / lower / upper / total for both calls,
inner path-steps and asset-steps per second, the bounds.  d = 1 is additionally timed with q = 0, where it returns the
vanilla call's bits: the two then run the same instruction mix.  usage: time_basket_bounds.py [reps] [N] [d ...]"""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 9
ds = [int(v) for v in sys.argv[3:]] or [1, 2, 4, 8]
ctx = _ffi.default_context(0)
p = _ffi.make_params(semantics="two_pass", is_put=False, n_paths=100_000, n_steps=N, S0=100.0, K=100.0, r=0.05, sigma=0.2,
                     T=3.0, seed=42)
KEYS = ("ms_fit", "ms_lower", "ms_upper", "ms_total")


def med(rs, k):
    return st.median(r[k] for r in rs)


def run(d, q):
    b = _ffi.make_basket([100.0] * d, [0.2] * d, [q] * d, [1.0] * d, None, "best-of")
    ctx.price_american_basket_bounds(p, b)  # warm-up: code objects, workspaces
    ctx.price_american_bounds(p)
    rb, rv = [], []
    for _ in range(reps):  # alternated: both see the same clocks and the same neighbours
        rb.append(ctx.price_american_basket_bounds(p, b))
        rv.append(ctx.price_american_bounds(p))
    r0, v0 = rb[0], rv[0]
    up_s = med(rb, "ms_upper") * 1e-3
    return dict(d=d, q=q, N=N, reps=reps, n_lower=r0["n_lower"], n_outer=r0["n_outer"], n_inner=r0["n_inner"],
                ms={k[3:]: med(rb, k) for k in KEYS}, vanilla_ms={k[3:]: med(rv, k) for k in KEYS},
                inner_path_steps=r0["inner_path_steps"], vanilla_inner_path_steps=v0["inner_path_steps"],
                inner_path_steps_per_s=r0["inner_path_steps"] / up_s, inner_asset_steps_per_s=d * r0["inner_path_steps"] / up_s,
                vanilla_inner_path_steps_per_s=v0["inner_path_steps"] / (med(rv, "ms_upper") * 1e-3),
                lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"],
                same_bits_as_vanilla=bool(q == 0.0 and d == 1 and (r0["lower"], r0["upper"]) == (v0["lower"], v0["upper"])))


for d in ds:
    if d == 1:
        print(json.dumps(run(1, 0.0)), flush=True)
    print(json.dumps(run(d, 0.1)), flush=True)

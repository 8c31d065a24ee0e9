"""HIP-event cost of omc_price_american_bounds for the headline GBM put (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1;
textbook policy fitted on 100,000 paths; default sizes n_lower 1M, n_outer 8192, n_inner 1024) at N = 50 and N = 252.
Prints one JSON line per N: median event times of fit / lower / upper / total, inner_path_steps and inner path-steps per
second, the bounds, and the in-sample prices of the library's three poly flows (1M paths, seed 42) next to them --
where the library's default answer sits against the Bermudan value.  usage: time_bounds.py [reps] [N ...]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_bounds.py`."""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
Ns = [int(v) for v in sys.argv[2:]] or [50, 252]
ctx = _ffi.default_context(0)
for N in Ns:
    p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=100_000, n_steps=N, seed=42)
    ctx.price_american_bounds(p)  # warm-up: code objects, workspaces
    rs = [ctx.price_american_bounds(p) for _ in range(reps)]
    med = lambda k: st.median(r[k] for r in rs)  # noqa: E731
    r0 = rs[0]
    flows = {}
    for sem in ("reference", "two_pass", "textbook"):
        q = _ffi.make_params(semantics=sem, is_put=True, n_paths=1_000_000, n_steps=N, seed=42)
        flows[sem] = ctx.price_american(q)["price"]
    out = dict(N=N, reps=reps, n_lower=r0["n_lower"], n_outer=r0["n_outer"], n_inner=r0["n_inner"],
               ms=dict(fit=med("ms_fit"), lower=med("ms_lower"), upper=med("ms_upper"), total=med("ms_total")),
               inner_path_steps=r0["inner_path_steps"],
               inner_path_steps_per_s=r0["inner_path_steps"] / (med("ms_upper") * 1e-3),
               lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"],
               ci=[r0["ci_lo"], r0["ci_hi"]], n_exercised_lower=r0["n_exercised_lower"],
               in_sample_flows=flows)
    print(json.dumps(out), flush=True)

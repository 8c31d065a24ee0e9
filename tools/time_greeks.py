"""HIP-event cost of one omc_price_american_greeks call against one omc_price_american at 1M x 252 (GBM put: folded storage
by default; Heston put: full storage), the two alternated in one process.  Prints one JSON line per case: median event
times of the whole call (paths + LSM) and of its kernels, and their ratio.  usage: time_greeks.py [reps] [M N]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_greeks.py`."""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
M, N = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1_000_000, 252)
ctx = _ffi.default_context(0)
cases = {
    "gbm_put": dict(model="gbm"),
    "heston_put": dict(model="heston", v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7, heston_scheme=0),
}
for name, kw in cases.items():
    p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=42, **kw)
    ctx.price_american(p)
    ctx.price_american_greeks(p)  # warm-up: code objects, workspaces
    a, g = [], []
    for _ in range(reps):
        a.append(ctx.price_american(p))
        g.append(ctx.price_american_greeks(p))
    med = lambda rs, k: st.median(r[k] for r in rs)  # noqa: E731
    out = dict(case=name, M=M, N=N, reps=reps, folded=g[0]["folded"],
               price_ms=dict(total=med(a, "ms_total"), paths=med(a, "ms_paths"), pass1=med(a, "ms_pass1"),
                             pass2=med(a, "ms_pass2")),
               greeks_ms=dict(total=med(g, "ms_total"), paths=med(g, "ms_paths"), pass1=med(g, "ms_pass1"),
                              sweep=med(g, "ms_greeks")),
               ratio=med(g, "ms_total") / med(a, "ms_total"),
               greeks={k: g[0][k] for k in ("price", "delta", "gamma", "vega", "rho", "theta")})
    print(json.dumps(out), flush=True)

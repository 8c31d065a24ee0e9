"""HIP-event cost of omc_price_american_basket_greeks at 1M x 252, put, the variants alternated in
one process, medians of `reps` calls (default 5) after 2 warm-up rounds, for an arithmetic basket of d = 1, 2, 4, 8 assets
(equicorrelation 0.3, weights 1 / d):
  p<d>   omc_price_american_basket: the pricing (generator, pass 1, pass 2)
  g<d>   omc_price_american_basket_greeks, want_gamma = 0: generator, pass 1, the sweep with the base chains only
  G<d>   the same with want_gamma = 1: 2 (2 d + 1) chains per pair
and beside d = 1
  v1     omc_price_american_greeks on full storage (option "fold_antithetic" = 0): the sweep that reads the stored matrix
Prints one JSON line: median event times per variant (total, paths, pass 1, pass 2 / the Greeks sweep), the run-to-run
spread of p1, the ratios of each Greeks call to its pricing, and the sweep's share of its call.
usage: time_basket_greeks.py [reps] [M N]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_basket_greeks.py`."""
import json
import os
import statistics as st
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
M, N = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1_000_000, 252)
ctx = _ffi.default_context(0)
p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=42)


def basket(d):
    rho = np.full((d, d), 0.3) + 0.7 * np.eye(d)
    return _ffi.make_basket([100.0] * d, [0.2] * d, [0.0] * d, [1.0 / d] * d, rho, "basket")


def full(fn):
    ctx.set_option("fold_antithetic", 0)
    try:
        return fn()
    finally:
        ctx.set_option("fold_antithetic", 1)


variants = {}
for d in (1, 2, 4, 8):
    b = basket(d)
    variants[f"p{d}"] = (lambda b: lambda: ctx.price_american_basket(p, b))(b)
    variants[f"g{d}"] = (lambda b: lambda: ctx.price_american_basket_greeks(p, b, gamma=False))(b)
    variants[f"G{d}"] = (lambda b: lambda: ctx.price_american_basket_greeks(p, b, gamma=True))(b)
    if d == 1:
        variants["v1"] = lambda: full(lambda: ctx.price_american_greeks(p))
runs = {k: [] for k in variants}
for i in range(2 + reps):
    for k, fn in variants.items():
        r = fn()
        if i >= 2:
            runs[k].append(r)


def med(k, key):
    return st.median(r[key] for r in runs[k])


out = dict(M=M, N=N, reps=reps)
for k in variants:
    out[k] = dict(total=med(k, "ms_total"), paths=med(k, "ms_paths"), pass1=med(k, "ms_pass1"), price=runs[k][0]["price"])
    if k[0] == "p":
        out[k]["pass2"] = med(k, "ms_pass2")
    else:
        out[k]["greeks"] = med(k, "ms_greeks")
        out[k]["greeks_share"] = out[k]["greeks"] / out[k]["total"]
tp = [r["ms_total"] for r in runs["p1"]]
out["p1_spread_ms"] = max(tp) - min(tp)
for d in (1, 2, 4, 8):
    for g in ("g", "G"):
        out[f"{g}{d}_over_p{d}_total"] = out[f"{g}{d}"]["total"] / out[f"p{d}"]["total"]
        out[f"{g}{d}_sweep_over_p{d}_paths"] = out[f"{g}{d}"]["greeks"] / out[f"p{d}"]["paths"]
out["v1_over_p1_total"] = out["v1"]["total"] / out["p1"]["total"]
print(json.dumps(out), flush=True)

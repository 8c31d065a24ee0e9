"""HIP-event cost of the Asian index kinds, the calls alternated in one process, medians of `reps`
calls (default 5) after warm-up rounds.

Pricing, omc_price_american_basket at M x N (default 1M x 252), put, d = 1, 2, 4 (equicorrelation 0.3, weights 1 / d):
  basket     kind OMC_BASKET_ARITHMETIC, the comparator: the same assets, the index without a state
  asian      kind OMC_BASKET_ASIAN_ARITHMETIC: one add and one multiply more per partner and step
  asian_geo  kind OMC_BASKET_ASIAN_GEOMETRIC: a log2, an add, a multiply and an exp2 more
-> the generator alone (ms_basket_paths) and the whole call, and their ratios to `basket`.

Bounds at the default sizes (n_lower 1M, n_outer 8192, n_inner 1024; nine dates, T = 3, textbook policy on 100,000 paths),
two assets, call:
  basket_index / asian_index     omc_price_american_basket_bounds at kind "basket" and kind "asian"
  bestof_runnerup / asian_spot   omc_price_american_basket_bounds_runnerup at best-of and kind "asian"
-> median fit / lower / upper / total, inner path-steps, path-steps per second of the upper phase, and the ratios.
Prints one JSON line per block.  usage: time_asian.py [reps] [M N]"""
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


def basket(d, kind, q=0.0):
    rho = np.full((d, d), 0.3) + 0.7 * np.eye(d)
    w = [1.0] * d if kind == "best-of" else [1.0 / d] * d
    return _ffi.make_basket([100.0] * d, [0.2] * d, [q] * d, w, rho, kind)


def alternate(calls, warm=2):
    runs = {k: [] for k in calls}
    for i in range(warm + reps):  # alternated: all see the same clocks and the same neighbours
        for k, f in calls.items():
            r = f()
            if i >= warm:
                runs[k].append(r)
    return runs


# ---------------------------------------------------------------------------------------------- pricing
p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=42)
KINDS = dict(basket="basket", asian="asian", asian_geo="asian-geometric")
for d in (1, 2, 4):
    calls = {k: (lambda b: lambda: ctx.price_american_basket(p, b))(basket(d, kind)) for k, kind in KINDS.items()}
    runs = alternate(calls)
    out = dict(block="pricing", d=d, M=M, N=N, reps=reps)
    for k, rs in runs.items():
        paths = [r["ms_basket_paths"] for r in rs]
        out[k] = dict(paths=st.median(paths), total=st.median(r["ms_total"] for r in rs), paths_spread=max(paths) - min(paths),
                      price=rs[0]["price"])
    for k in ("asian", "asian_geo"):
        out[k + "_over_basket_paths"] = out[k]["paths"] / out["basket"]["paths"]
        out[k + "_over_basket_total"] = out[k]["total"] / out["basket"]["total"]
    print(json.dumps(out), flush=True)

# ---------------------------------------------------------------------------------------------- bounds
NB = 9
pb = _ffi.make_params(semantics="two_pass", is_put=False, n_paths=100_000, n_steps=NB, S0=100.0, K=100.0, r=0.05, sigma=0.2,
                      T=3.0, seed=42)
KEYS = ("ms_fit", "ms_lower", "ms_upper", "ms_total")
calls = dict(basket_index=lambda: ctx.price_american_basket_bounds(pb, basket(2, "basket", 0.1)),
             asian_index=lambda: ctx.price_american_basket_bounds(pb, basket(2, "asian", 0.1)),
             bestof_runnerup=lambda: ctx.price_american_basket_bounds(pb, basket(2, "best-of", 0.1),
                                                                      regressors="index+runner-up"),
             asian_spot=lambda: ctx.price_american_basket_bounds(pb, basket(2, "asian", 0.1), regressors="index+spot"))
runs = alternate(calls, warm=1)
out = dict(block="bounds", d=2, N=NB, reps=reps)
for k, rs in runs.items():
    ms = {key[3:]: st.median(r[key] for r in rs) for key in KEYS}
    out[k] = dict(ms=ms, inner_path_steps=rs[0]["inner_path_steps"],
                  inner_path_steps_per_s=rs[0]["inner_path_steps"] / (ms["upper"] * 1e-3), lower=rs[0]["lower"],
                  se_lower=rs[0]["se_lower"], upper=rs[0]["upper"], se_upper=rs[0]["se_upper"])
    out["n_lower"], out["n_outer"], out["n_inner"] = rs[0]["n_lower"], rs[0]["n_outer"], rs[0]["n_inner"]
for a, b in (("asian_index", "basket_index"), ("asian_spot", "bestof_runnerup"), ("asian_spot", "asian_index")):
    out[f"{a}_over_{b}_total"] = out[a]["ms"]["total"] / out[b]["ms"]["total"]
    out[f"{a}_over_{b}_steps_per_s"] = out[a]["inner_path_steps_per_s"] / out[b]["inner_path_steps_per_s"]
print(json.dumps(out), flush=True)

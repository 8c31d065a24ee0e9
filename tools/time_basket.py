"""HIP-event cost of omc_price_american_basket at 1M x 252, put, the variants alternated in one
process, medians of `reps` calls (default 5) after 2 warm-up rounds:
  a     omc_price_american, option "fold_antithetic" = 0: the comparator, one GBM asset on the full-storage sweeps
  d1 .. omc_price_american_basket, arithmetic basket of d = 1, 2, 4, 8 assets (equicorrelation 0.3, weights 1 / d)
  g4    the same at d = 4, geometric (the extra exp2 per path and step of the index's own state)
  b4    the same at d = 4, best-of
Prints one JSON line: median event times per variant, the run-to-run spread of a, the ratios to a, and the kernel
instantiation <D, VEC> each basket variant ran (VEC from the rule of launch_basket_paths: at most 4 / 2 / 1 pairs per lane
for d <= 2 / <= 4 / <= 8, halved until the pair count and the leading dimension are multiples of it).
usage: time_basket.py [reps] [M N]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_basket.py`."""
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


def basket(d, kind="basket"):
    rho = np.full((d, d), 0.3) + 0.7 * np.eye(d)
    w = [1.0 / d] * d if kind != "best-of" else [1.0] * d
    return _ffi.make_basket([100.0] * d, [0.2] * d, [0.0] * d, w, rho, kind)


def full(fn):
    ctx.set_option("fold_antithetic", 0)
    try:
        return fn()
    finally:
        ctx.set_option("fold_antithetic", 1)


def vec_of(d):
    v, ld = (4 if d <= 2 else 2 if d <= 4 else 1), (M + 63) // 64 * 64  # the library's own matrix: ld padded to 64
    while v > 1 and ((M // 2) % v or ld % v):
        v //= 2
    return v


variants = {"a_american_full": lambda: full(lambda: ctx.price_american(p))}
for d in (1, 2, 4, 8):
    variants[f"d{d}_basket"] = (lambda b: lambda: ctx.price_american_basket(p, b))(basket(d))
variants["g4_geometric"] = (lambda b: lambda: ctx.price_american_basket(p, b))(basket(4, "geometric"))
variants["b4_best_of"] = (lambda b: lambda: ctx.price_american_basket(p, b))(basket(4, "best-of"))
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
    out[k] = dict(total=med(k, "ms_total"), paths=med(k, "ms_paths"), pass1=med(k, "ms_pass1"), pass2=med(k, "ms_pass2"),
                  folded=runs[k][0]["folded"], price=runs[k][0]["price"])
    if k != "a_american_full":
        d = runs[k][0]["n_assets"]
        out[k]["kernel"] = f"basket_paths_kernel<{d}, {vec_of(d)}, false>"
ta = [r["ms_total"] for r in runs["a_american_full"]]
pa = [r["ms_paths"] for r in runs["a_american_full"]]
out["a_spread_ms"] = max(ta) - min(ta)
out["a_paths_spread_ms"] = max(pa) - min(pa)
for k in variants:
    if k != "a_american_full":
        tag = k.split("_")[0]
        out[tag + "_over_a_total"] = out[k]["total"] / out["a_american_full"]["total"]
        out[tag + "_over_a_paths"] = out[k]["paths"] / out["a_american_full"]["paths"]
print(json.dumps(out), flush=True)

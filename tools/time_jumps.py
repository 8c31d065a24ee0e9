"""HIP-event cost of omc_price_american_jump at 1M x 252, GBM put, the variants alternated in one
process, medians of `reps` calls (default 5) after 2 warm-up rounds:
  a  omc_price_american, option "fold_antithetic" = 0: the comparator, the full-storage sweeps the jump pricing uses
  b  omc_price_american_div, four quarterly cash dividends: the other generator of this kind
  c  omc_price_american_jump, lambda = 1, mu_j = -0.1, sigma_j = 0.15 (Merton)
  d  the same with lambda = 50
  z  the same with lambda = 1e-4: the jump branch all but never taken, so z - a is the count block and its compares alone
  h  omc_price_american on Heston paths: what the Heston generator costs relative to GBM, the yardstick for c
  e  omc_price_american_jump on Heston paths, lambda = 1 (Bates)
Prints one JSON line: median event times per variant, the run-to-run spread of a, and the ratios to a.
usage: time_jumps.py [reps] [M N]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_jumps.py`."""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
M, N = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1_000_000, 252)
ctx = _ffi.default_context(0)
p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=42)
ph = _ffi.make_params(model="heston", semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=42)
quarterly = [(0.25 * (i + 1) - 0.125, 0.75, "cash") for i in range(4)]


def full(fn):
    ctx.set_option("fold_antithetic", 0)
    try:
        return fn()
    finally:
        ctx.set_option("fold_antithetic", 1)


variants = {
    "a_american_full": lambda: full(lambda: ctx.price_american(p)),
    "b_dividends_cash4": lambda: ctx.price_american_div(p, 0.0, quarterly),
    "c_merton_lambda1": lambda: ctx.price_american_jump(p, (1.0, -0.1, 0.15), 0.0),
    "d_merton_lambda50": lambda: ctx.price_american_jump(p, (50.0, -0.1, 0.15), 0.0),
    "z_merton_lambda1e-4": lambda: ctx.price_american_jump(p, (1e-4, -0.1, 0.15), 0.0),
    "h_american_heston": lambda: ctx.price_american(ph),
    "e_bates_lambda1": lambda: ctx.price_american_jump(ph, (1.0, -0.1, 0.15), 0.0),
}
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
ta = [r["ms_total"] for r in runs["a_american_full"]]
pa = [r["ms_paths"] for r in runs["a_american_full"]]
out["a_spread_ms"] = max(ta) - min(ta)
out["a_paths_spread_ms"] = max(pa) - min(pa)
for k in variants:
    if k != "a_american_full":
        out[k[0] + "_over_a_total"] = out[k]["total"] / out["a_american_full"]["total"]
        out[k[0] + "_over_a_paths"] = out[k]["paths"] / out["a_american_full"]["paths"]
out["e_over_h_paths"] = out["e_bates_lambda1"]["paths"] / out["h_american_heston"]["paths"]
print(json.dumps(out), flush=True)

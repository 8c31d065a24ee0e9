"""HIP-event cost of omc_price_american_div at 1M x 252, GBM put, the variants alternated in one
process, medians of `reps` calls (default 5) after 2 warm-up rounds:
  a  omc_price_american, option "fold_antithetic" = 0: the comparator, the full-storage sweeps the dividend pricing uses
  b  omc_price_american_div, four quarterly cash dividends
  c  omc_price_barrier, discrete down-and-out American (tools/time_barrier.py): a yardstick -- its generator does more
     per step (knock state, European sums), so b should not exceed it
  d  yield only on the default storage against omc_price_american on the default storage (the same kernels)
Prints one JSON line: median event times per variant, the run-to-run spread of a, and the ratios.
usage: time_dividends.py [reps] [M N]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_dividends.py`."""
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
    "c_barrier_down_out": lambda: ctx.price_barrier(p, "down-and-out", 90.0, monitoring="discrete", american=True),
    "d_american_default": lambda: ctx.price_american(p),
    "d_yield_default": lambda: ctx.price_american_div(p, 0.03, []),
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
    paths = "ms_barrier_paths" if k.startswith("c_") else "ms_paths"
    out[k] = dict(total=med(k, "ms_total"), paths=med(k, paths), pass1=med(k, "ms_pass1"), pass2=med(k, "ms_pass2"),
                  folded=runs[k][0]["folded"], price=runs[k][0]["price"])
ta = [r["ms_total"] for r in runs["a_american_full"]]
out["a_spread_ms"] = max(ta) - min(ta)
out["b_over_a_total"] = out["b_dividends_cash4"]["total"] / out["a_american_full"]["total"]
out["b_over_a_paths"] = out["b_dividends_cash4"]["paths"] / out["a_american_full"]["paths"]
out["b_over_c_total"] = out["b_dividends_cash4"]["total"] / out["c_barrier_down_out"]["total"]
out["b_over_c_paths"] = out["b_dividends_cash4"]["paths"] / out["c_barrier_down_out"]["paths"]
out["d_gap_ms"] = out["d_yield_default"]["total"] - out["d_american_default"]["total"]
print(json.dumps(out), flush=True)

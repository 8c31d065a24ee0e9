#!/usr/bin/env python3
"""Cost of the price bounds with an exercise schedule (option "bounds_exercise_every").

The ATM put (S0 = K = 100, r = 0.05, T = 1; textbook policy fitted on 100,000 paths), default sizes (n_lower 1M, n_outer
8192, n_inner 1024), for GBM (sigma 0.2) and Heston scheme 1 (v0 = theta = 0.04, kappa 2, xi 0.3, rho -0.7).  Three calls
alternate in one process, HIP-event times (omc_bounds.ms_*), medians of --reps:
  (a) N = 252, exercise_every = 21: the monthly Bermudan on the daily grid
  (b) N = 50, every date: the call the library has had, the yardstick
  (c) N = 252, option 0, (a)'s holed table as a given policy: how the lower bound and Q^ of (a) could be had without the
      scheduled kernels -- inner simulations at all 252 dates; what the items at unscheduled dates cost
and prints the brackets, inner_path_steps and path-steps per second.

  python tools/time_bounds_schedule.py [--reps 5] [--n-outer-c 8192] [-o profiles/bounds_schedule_time.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from options_model_amd import _ffi  # noqa: E402

HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
EXPECTED = """Expectation, read from the code before the run:
  (a) takes at most n_outer n_inner sum_j (N - tau_j) = 8192 * 1024 * 1638 = 1.37e10 inner path-steps (tau_j = 0, 21, .., 231),
      about 1.6 times (b)'s 8.5e9 to 8.7e9, and fewer where the policy stops paths early;
  its rate per path-step should be at or above (b)'s: between two scheduled dates a step skips the LDS read, the two table
      compares and the bookkeeping of bd_mark, and a pair can only finish at a scheduled date, so fewer draws are cut short;
  (c) simulates from all 252 dates to the next scheduled stop, about 252 / 12 = 21 times (a)'s items and 10 to 20 times its steps."""


def params(model, N):
    if model == "gbm":
        return _ffi.make_params(model="gbm", is_put=True, semantics="two_pass", n_paths=100_000, n_steps=N, S0=100.0, K=100.0,
                                r=0.05, sigma=0.2, T=1.0, seed=42, stream=0)
    return _ffi.make_params(model="heston", heston_scheme=1, is_put=True, semantics="two_pass", n_paths=100_000, n_steps=N,
                            S0=100.0, K=100.0, r=0.05, sigma=0.0, T=1.0, seed=42, stream=0, **HP)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-lower", type=int, default=1_000_000)
    ap.add_argument("--n-outer", type=int, default=8192)
    ap.add_argument("--n-inner", type=int, default=1024)
    ap.add_argument("--n-outer-c", type=int, default=8192, help="outer paths of call (c); below --n-outer its times are scaled up")
    ap.add_argument("-o", "--output", default="-")
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    lines = [f"tools/time_bounds_schedule.py --reps {a.reps} on one MI355X: the ATM put (S0 = K = 100, r = 0.05, T = 1; textbook "
             f"policy fitted on 100,000 paths),", f"n_lower {a.n_lower}, n_outer {a.n_outer}, n_inner {a.n_inner}, HIP-event "
             f"medians of {a.reps} in ms; the three calls alternate in one process.", "", EXPECTED, "",
             f"  {'model':8s} {'call':28s} {'fit':>7s} {'lower':>7s} {'upper':>9s} {'total':>9s} {'inner path-steps':>17s} "
             f"{'path-steps/s':>13s}   bracket"]
    raw = []
    for model in ("gbm", "heston1"):
        price = ctx.price_american_bounds if model == "gbm" else ctx.price_american_bounds_heston
        sizes = dict(n_lower=a.n_lower, n_outer=a.n_outer, n_inner=a.n_inner)
        first = price(params(model, 252), exercise_every=21, **sizes)
        calls = {
            "a N=252 every 21st date": lambda: price(params(model, 252), exercise_every=21, **sizes),
            "b N=50 every date": lambda: price(params(model, 50), **sizes),
            "c N=252 all dates, a's table": lambda: price(params(model, 252), policy="given", betas=first["betas"],
                                                          **dict(sizes, n_outer=a.n_outer_c)),
        }
        for fn in calls.values():  # warm-up: allocations, the discount tables
            fn()
        runs = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                runs[name].append(fn())
        for name, rs in runs.items():
            scale = a.n_outer / a.n_outer_c if name.startswith("c") else 1.0
            ms = {k: statistics.median(r["ms_" + k] for r in rs) for k in ("fit", "lower", "upper", "total")}
            d = rs[-1]
            steps = d["inner_path_steps"]
            rate = steps / (ms["upper"] * 1e-3)
            note = f"  (n_outer {a.n_outer_c}; upper and total x {scale:g})" if scale != 1.0 else ""
            ms_u, ms_t = ms["upper"] * scale, ms["fit"] + ms["lower"] + ms["upper"] * scale
            lines.append(f"  {model:8s} {name:28s} {ms['fit']:7.3f} {ms['lower']:7.3f} {ms_u:9.3f} {ms_t:9.3f} {int(steps * scale):17d} "
                         f"{rate:13.3e}   [{d['lower']:.4f} ({d['se_lower']:.4f}), {d['upper']:.4f} ({d['se_upper']:.4f})]{note}")
            raw.append(dict(model=model, call=name, reps=a.reps, ms=ms, n_outer=d["n_outer"], n_inner=d["n_inner"],
                            inner_path_steps=steps, inner_path_steps_per_s=rate, lower=d["lower"], se_lower=d["se_lower"],
                            upper=d["upper"], se_upper=d["se_upper"], n_exercised_lower=d["n_exercised_lower"]))
        A, B, Cc = (next(r for r in raw if r["model"] == model and r["call"].startswith(c)) for c in "abc")
        sc = a.n_outer / a.n_outer_c
        lines.append(f"  {model:8s} upper a / b {A['ms']['upper'] / B['ms']['upper']:.3f}; steps a / b "
                     f"{A['inner_path_steps'] / B['inner_path_steps']:.3f}; rate a / b "
                     f"{A['inner_path_steps_per_s'] / B['inner_path_steps_per_s']:.3f}; upper c / a "
                     f"{Cc['ms']['upper'] * sc / A['ms']['upper']:.2f}; steps c / a "
                     f"{Cc['inner_path_steps'] * sc / A['inner_path_steps']:.2f}; lower of c == lower of a: "
                     f"{Cc['lower'] == A['lower']}")
        lines.append("")
    ctx.close()
    lines += ["The raw lines:"] + [json.dumps(r) for r in raw]
    text = "\n".join(lines) + "\n"
    if a.output == "-":
        sys.stdout.write(text)
    else:
        with open(a.output, "w") as f:
            f.write(text)
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

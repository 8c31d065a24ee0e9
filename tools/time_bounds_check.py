#!/usr/bin/env python3
"""Cost and bracket of the price bounds with sub-optimality checking (option "bounds_suboptimality").

(A) The README's ATM GBM put on 50 dates (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1; textbook policy fitted on 100,000
paths), n_lower 1M, n_outer 8192: plain and with the control variate, at n_inner 1024 and 16, with the check off (0), "payoff"
(1) and "european" (2).  (B) The README's Heston put on 50 dates (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7) and (C)
its two-asset max-call benchmark (nine dates, S0 = 100, K = 100, r = 0.05, q = 0.1, sigma = 0.2, T = 3), default sizes, with
the check off and "payoff".  The calls of a game alternate in one process; HIP-event times (omc_bounds.ms_*), medians of --reps.
The comparison is mode 0 in the same run.  Beside the times: the share of inner path-steps and of ms_upper that is left, and
the bracket.

  python tools/time_bounds_check.py [--reps 5] [-o profiles/bounds_check_time.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from options_model_amd import _ffi  # noqa: E402

EXPECTED = """Expectation, written before the first run -- the float64 numpy restatement on 12 dates, 256 outer and 16 inner paths
(items kept / inner steps kept, payoff | European):
      put S0 = 100   0.509 / 0.482 | 0.257 / 0.221      put S0 = 90    0.779 / 0.749 | 0.519 / 0.380
      put S0 = 110   0.262 / 0.260 | 0.135 / 0.168      call S0 = 100  0.575 / 0.603 | 0.083 / 0.154 (policy scaled by 0.97)
  with no sample above the unchecked one (largest excess 1.4e-14) and the lower bound untouched.  On 50 dates the shares should
  be close to those of the ATM put: about a half of the inner steps left by the payoff check, a quarter by the European one.
  ms_upper should follow the steps at n_inner 1024, where the sweep is nearly all of it; less than in proportion, because the
  kept items of a date no longer fill the grid evenly and the longest items (date 0, every path) are all kept.  At n_inner 16
  the sweep is short: the mark kernel, the one-workgroup compaction (409,600 items: 25 rounds of 16,384) and the memset of Q^
  are a fixed cost of some tens of microseconds that the check adds, so the gain there should be smaller, and may be none for
  the plain sweep, whose waves are mostly idle lanes at 8 pairs an item.  The lower bound and ms_lower must not move.
What the first run showed, and what was changed after it: the shares at 50 dates are smaller than expected (0.389 and 0.086 of
  the steps), ms_upper follows them less than in proportion as expected, and the one-workgroup compaction cost about 0.13 ms --
  at n_inner 16 the controlled call was SLOWER with the payoff check (0.438 against 0.373 ms) and no faster with the European
  one (0.378).  The compaction is now a workgroup per date on per-date counts that the mark kernel leaves (DESIGN.md 27.3);
  the figures below are that version's."""


def gbm_params():
    return _ffi.make_params(model="gbm", is_put=True, semantics="two_pass", n_paths=100_000, n_steps=50, S0=100.0, K=100.0,
                            r=0.05, sigma=0.2, T=1.0, seed=42, stream=0)


def heston_params():
    return _ffi.make_params(model="heston", heston_scheme=0, is_put=True, semantics="two_pass", n_paths=100_000, n_steps=50,
                            S0=100.0, K=100.0, r=0.05, sigma=0.0, T=1.0, seed=42, stream=0, v0=0.04, kappa=2.0, theta=0.04,
                            xi=0.3, rho=-0.7)


def maxcall():
    p = _ffi.make_params(model="gbm", is_put=False, semantics="two_pass", antithetic=True, n_paths=100_000, n_steps=9, S0=100.0,
                         K=100.0, r=0.05, sigma=0.2, T=3.0, seed=42, stream=0)
    return p, _ffi.make_basket([100.0, 100.0], [0.2, 0.2], [0.1, 0.1], [1.0, 1.0], None, "best-of")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-lower", type=int, default=1_000_000)
    ap.add_argument("--n-outer", type=int, default=8192)
    ap.add_argument("-o", "--output", default="-")
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    sizes = dict(n_lower=a.n_lower, n_outer=a.n_outer)
    lines = [f"tools/time_bounds_check.py --reps {a.reps} on one MI355X: n_lower {a.n_lower}, n_outer {a.n_outer}, HIP-event "
             f"medians of {a.reps} in ms;", "the calls of a game alternate in one process; the comparison is the check off (0) "
             "in the same run.", "", EXPECTED, "",
             f"  {'game':34s} {'check':>8s} {'lower':>7s} {'upper':>9s} {'total':>9s} {'x upper':>8s} {'inner path-steps':>17s} "
             f"{'steps kept':>10s}   bracket"]
    raw = []
    games = []
    pg, ph = gbm_params(), heston_params()
    pb, bb = maxcall()
    for cv in (False, True):
        for n_inner in (1024, 16):
            games.append((f"A GBM put N=50 {'controlled' if cv else 'plain'} {n_inner}", (0, 1, 2),
                          lambda m, cv=cv, n=n_inner: ctx.price_american_bounds(pg, n_inner=n, control_variate=cv,
                                                                                suboptimality_check=_ffi.BOUND_CHECKS[m], **sizes)))
    games.append(("B Heston put N=50 1024", (0, 1),
                  lambda m: ctx.price_american_bounds_heston(ph, n_inner=1024, suboptimality_check=_ffi.BOUND_CHECKS[m], **sizes)))
    games.append(("C two-asset max-call N=9 1024", (0, 1),
                  lambda m: ctx.price_american_basket_bounds(pb, bb, n_inner=1024, suboptimality_check=_ffi.BOUND_CHECKS[m],
                                                             **sizes)))
    for game, modes, fn in games:
        for m in modes:  # warm-up: allocations, the discount tables
            fn(m)
        runs = {m: [] for m in modes}
        for _ in range(a.reps):
            for m in modes:
                runs[m].append(fn(m))
        ms0 = steps0 = None
        for m in modes:
            rs = runs[m]
            ms = {k: statistics.median(r["ms_" + k] for r in rs) for k in ("fit", "lower", "upper", "total")}
            d = rs[-1]
            steps = d["inner_path_steps"]
            if m == 0:
                ms0, steps0 = ms, steps
            lines.append(f"  {game:34s} {_ffi.BOUND_CHECKS[m]:>8s} {ms['lower']:7.3f} {ms['upper']:9.3f} {ms['total']:9.3f} "
                         f"{ms['upper'] / ms0['upper']:8.3f} {steps:17d} {steps / steps0:10.3f}"
                         f"   [{d['lower']:.4f} ({d['se_lower']:.5f}), {d['upper']:.4f} ({d['se_upper']:.5f})]")
            raw.append(dict(game=game, check=_ffi.BOUND_CHECKS[m], reps=a.reps, ms=ms, n_inner=d["n_inner"],
                            inner_path_steps=steps, steps_kept=steps / steps0, upper_time_ratio=ms["upper"] / ms0["upper"],
                            lower=d["lower"], se_lower=d["se_lower"], upper=d["upper"], se_upper=d["se_upper"]))
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

#!/usr/bin/env python3
"""Cost and bracket of the GBM price bounds with the Black-Scholes control variate (option "bounds_control_variate",
DESIGN.md section 26).

The ATM put (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1; textbook policy fitted on 100,000 paths), n_lower 1M, n_outer 8192,
for (A) the all-dates game on 50 dates and (B) the monthly schedule on 252 (exercise_every = 21).  The calls alternate in one
process, HIP-event times (omc_bounds.ms_*), medians of --reps:
  plain at n_inner 1024; controlled at n_inner 1024, 256, 64 and 16
  and, at n_inner 16 and 1024, the controlled inner sweep with one item per wave (G = 64) whatever n_inner (option
  "bounds_cv_form" = 1) against the lane groups.
The first runs of this tool also timed the other place of the evaluation -- a finished pair evaluated in the iteration it ends,
against finished lanes that wait -- and the number of waiting lanes; waiting won, 32 lanes were chosen afterwards, and the
kernels that evaluate at the stop are no longer built.  Those figures are kept in profiles/bounds_cv_resource_usage.txt and
DESIGN.md sections 6.4 and 26.4.
It prints ms_upper, ms_total, inner path-steps per second, the bracket and both standard errors, and the smallest controlled
n_inner whose upper bound is at or below the plain call's, with what the whole call then costs.

  python tools/time_bounds_cv.py [--reps 5] [-o profiles/bounds_cv_time.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from options_model_amd import _ffi  # noqa: E402

EXPECTED = """Expectation, written before the first run (which still had both places of the evaluation, and 16 waiting lanes):
  the controlled call takes exactly the plain call's inner path-steps at the same n_inner (the same paths and stops), so at
      n_inner 1024 its upper sweep costs the plain sweep plus the evaluations: a pair that stops before expiry pays a float64
      log and two erfc per such partner, a few hundred instructions against the ~60 per step of a pair that runs ~25 steps,
      under a mask that the wave's other lanes sit out -- expected 1.3 to 2 times the plain upper sweep at equal n_inner,
      more if the inner kernel's 91 to 96 VGPRs (5 waves per SIMD against the plain kernel's 72 / 7) cost latency hiding;
  inner path-steps fall in proportion to n_inner, and ms_upper with them until the outer paths, the walk and the launch
      remain: n_inner 64 should cost about a tenth of the plain upper sweep, n_inner 16 less than that;
  lane groups: at n_inner 16 one item per wave leaves 56 of 64 lanes without a pair, so G = 8 should be several
      times faster there; at n_inner 1024 both are G = 64 and must cost the same;
  evaluation: letting finished lanes wait (16 of a wave, or until none is live) trades idle lanes for fewer executions of the
      evaluation under a thin mask; which wins is not clear from the code -- at n_inner 16 (G = 8, one pair per lane, no
      refill) the two forms should be close, at 1024 the refill gives waiting lanes a cost;
  the bracket: se_lower falls by about sqrt(60) = 8, and the controlled upper bound at n_inner 16 to 64 should sit at or
      below the plain one at 1024 (the float64 CPU experiment of the issue: 6.10 at 16 against 6.11 plain at 1024)."""


def params(N):
    return _ffi.make_params(model="gbm", is_put=True, semantics="two_pass", n_paths=100_000, n_steps=N, S0=100.0, K=100.0,
                            r=0.05, sigma=0.2, T=1.0, seed=42, stream=0)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-lower", type=int, default=1_000_000)
    ap.add_argument("--n-outer", type=int, default=8192)
    ap.add_argument("-o", "--output", default="-")
    a = ap.parse_args()
    ctx = _ffi.Context(0)
    lines = [f"tools/time_bounds_cv.py --reps {a.reps} on one MI355X: the ATM put (S0 = K = 100, r = 0.05, sigma = 0.2, T = 1; "
             f"textbook policy fitted on", f"100,000 paths), n_lower {a.n_lower}, n_outer {a.n_outer}, HIP-event medians of "
             f"{a.reps} in ms; the calls of a game alternate in one process.", "", EXPECTED, "",
             f"  {'game':22s} {'call':32s} {'lower':>7s} {'upper':>9s} {'total':>9s} {'inner path-steps':>17s} {'path-steps/s':>13s}"
             f"   bracket"]
    raw = []
    for game, N, every in (("A N=50 every date", 50, 0), ("B N=252 every 21st", 252, 21)):
        def call(n_inner, cv, form=0, N=N, every=every):
            def run():
                ctx.set_option("bounds_cv_form", form)
                try:
                    return ctx.price_american_bounds(params(N), n_lower=a.n_lower, n_outer=a.n_outer, n_inner=n_inner,
                                                     exercise_every=every, control_variate=cv)
                finally:
                    ctx.set_option("bounds_cv_form", 0)
            return run

        calls = {"plain 1024": call(1024, False)}
        for n in (1024, 256, 64, 16):
            calls[f"controlled {n}"] = call(n, True)
        for n in (1024, 16):
            calls[f"controlled {n}, G = 64"] = call(n, True, 1)
        for fn in calls.values():  # warm-up: allocations, the discount tables
            fn()
        runs = {name: [] for name in calls}
        for _ in range(a.reps):
            for name, fn in calls.items():
                runs[name].append(fn())
        rows = {}
        for name, rs in runs.items():
            ms = {k: statistics.median(r["ms_" + k] for r in rs) for k in ("fit", "lower", "upper", "total")}
            d = rs[-1]
            steps = d["inner_path_steps"]
            rate = steps / (ms["upper"] * 1e-3)
            lines.append(f"  {game:22s} {name:32s} {ms['lower']:7.3f} {ms['upper']:9.3f} {ms['total']:9.3f} {steps:17d} {rate:13.3e}"
                         f"   [{d['lower']:.4f} ({d['se_lower']:.5f}), {d['upper']:.4f} ({d['se_upper']:.5f})]")
            rows[name] = dict(game=game, call=name, reps=a.reps, ms=ms, n_inner=d["n_inner"], inner_path_steps=steps,
                              inner_path_steps_per_s=rate, lower=d["lower"], se_lower=d["se_lower"], upper=d["upper"],
                              se_upper=d["se_upper"], n_exercised_lower=d["n_exercised_lower"])
            raw.append(rows[name])
        plain = rows["plain 1024"]
        ok = [n for n in (16, 64, 256, 1024) if rows[f"controlled {n}"]["upper"] <= plain["upper"]]
        if ok:
            best = rows[f"controlled {ok[0]}"]
            lines.append(f"  {game}: the smallest controlled n_inner with upper <= the plain call's {plain['upper']:.4f}: {ok[0]} "
                         f"(upper {best['upper']:.4f}); the whole call then costs {best['ms']['total']:.3f} ms against "
                         f"{plain['ms']['total']:.3f} ms plain, x {plain['ms']['total'] / best['ms']['total']:.2f}")
        else:
            lines.append(f"  {game}: no controlled n_inner of 16 .. 1024 has upper <= the plain call's {plain['upper']:.4f}")
        for n in (1024, 16):
            base = rows[f"controlled {n}"]["ms"]["upper"]
            lines.append(f"  {game}: n_inner {n}: upper with lane groups {base:.3f} ms; with one item per wave (G = 64) "
                         f"{rows[f'controlled {n}, G = 64']['ms']['upper']:.3f} ms")
        lines.append(f"  {game}: controlled 1024 / plain 1024, upper sweep: x "
                     f"{rows['controlled 1024']['ms']['upper'] / plain['ms']['upper']:.3f}; se_lower plain / controlled: x "
                     f"{plain['se_lower'] / rows['controlled 1024']['se_lower']:.1f}")
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

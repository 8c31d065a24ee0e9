"""HIP-event cost of the Heston QE scheme at 1M x 252, the variants alternated in one process,
medians of `reps` calls (default 7) after 2 warm-up rounds.  Each variant is one omc_price_american on Heston paths (put,
two-pass flow): its `paths` time is the generator alone, its `total` the whole call's kernels.
  ft_A  scheme 1 (full truncation), set A: Feller satisfied, v0 = theta -- the comparator
  qe_A  scheme 3 (QE), set A: whole waves stay in the quadratic branch
  ft_B  scheme 1, set B: the Feller-violating `clamp` set (the Euler step costs the same; here for the ratio's denominator)
  qe_B  scheme 3, set B: most waves hold exponential lanes, so the erfc / log code runs
Prints a table and one JSON line: median event times per variant, the run-to-run spread of ft_A, and the ratios.
usage: time_heston_qe.py [reps] [M N]"""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
M, N = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1_000_000, 252)
SET_A = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
SET_B = dict(v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)
ctx = _ffi.default_context(0)


def params(scheme, hp):
    return _ffi.make_params(model="heston", heston_scheme=scheme, semantics="two_pass", is_put=True, n_paths=M, n_steps=N,
                            seed=42, **hp)


variants = {"ft_A": params(1, SET_A), "qe_A": params(3, SET_A), "ft_B": params(1, SET_B), "qe_B": params(3, SET_B)}
runs = {k: [] for k in variants}
for i in range(2 + reps):
    for k, p in variants.items():
        r = ctx.price_american(p)
        if i >= 2:
            runs[k].append(r)


def med(k, key):
    return st.median(r[key] for r in runs[k])


out = dict(M=M, N=N, reps=reps)
for k in variants:
    out[k] = dict(total=med(k, "ms_total"), paths=med(k, "ms_paths"), pass1=med(k, "ms_pass1"), pass2=med(k, "ms_pass2"),
                  price=runs[k][0]["price"])
out["ft_A_paths_spread_ms"] = max(r["ms_paths"] for r in runs["ft_A"]) - min(r["ms_paths"] for r in runs["ft_A"])
out["ft_A_total_spread_ms"] = max(r["ms_total"] for r in runs["ft_A"]) - min(r["ms_total"] for r in runs["ft_A"])
for s in "AB":
    out[f"qe_over_ft_paths_{s}"] = out[f"qe_{s}"]["paths"] / out[f"ft_{s}"]["paths"]
    out[f"qe_over_ft_total_{s}"] = out[f"qe_{s}"]["total"] / out[f"ft_{s}"]["total"]
out["qe_B_over_qe_A_paths"] = out["qe_B"]["paths"] / out["qe_A"]["paths"]
bytes_written = 4.0 * M * (N + 1)
print(f"{M:,} x {N}, put, S0 = K = 100, r = 0.05, T = 1, seed 42; medians of {reps} calls after 2 warm-up rounds")
print("variant   total ms  paths ms  pass1 ms  pass2 ms  paths GB/s       price")
for k in variants:
    o = out[k]
    print(f"{k:8s} {o['total']:9.4f} {o['paths']:9.4f} {o['pass1']:9.4f} {o['pass2']:9.4f} {bytes_written / o['paths'] / 1e6:11.0f} "
          f"{o['price']:11.6f}")
print(f"generator, QE over full truncation: set A {out['qe_over_ft_paths_A']:.3f}, set B {out['qe_over_ft_paths_B']:.3f}; "
      f"whole call: set A {out['qe_over_ft_total_A']:.3f}, set B {out['qe_over_ft_total_B']:.3f}; "
      f"QE set B over set A (the exponential branch): {out['qe_B_over_qe_A_paths']:.3f}")
print(f"run-to-run spread of ft_A (max - min): generator {out['ft_A_paths_spread_ms']:.4f} ms, total {out['ft_A_total_spread_ms']:.4f} ms")
print("raw: " + json.dumps(out), flush=True)

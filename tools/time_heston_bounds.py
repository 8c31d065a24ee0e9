"""HIP-event cost and bracket of omc_price_american_bounds_heston for the ATM put (S0 = K = 100, r = 0.05, T = 1; v0 = theta
= 0.04, kappa = 2, xi = 0.3, rho = -0.7; textbook policy fitted on 100,000 paths; default sizes n_lower 1M, n_outer 8192,
n_inner 1024) at N = 50, next to omc_price_american_bounds (GBM, sigma = 0.2) at the same sizes in the same process: the
calls alternate, the times are medians of the calls' own HIP events.  Prints one JSON line per Heston scheme -- the times
of both, the ratio of the upper phases and of the totals, inner path-steps per second of both, both brackets and their gaps
(upper - lower, absolute and relative to lower), the European put of the same scheme (4M paths), the in-sample prices of
the three poly flows -- and writes a table of them and the lines to profiles/heston_bounds_time.txt (or the path given).
usage: time_heston_bounds.py [reps] [out_path] [N]"""
import json
import os
import statistics as st
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "heston_bounds_time.txt")
N = int(sys.argv[3]) if len(sys.argv) > 3 else 50
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
ctx = _ffi.default_context(0)
rows = []
for scheme in ("reference", "full_truncation"):
    pg = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=100_000, n_steps=N, seed=42)
    ph = _ffi.make_params(model="heston", heston_scheme=scheme, semantics="two_pass", is_put=True, n_paths=100_000,
                          n_steps=N, seed=42, **HP)
    ctx.price_american_bounds(pg)  # warm-up: code objects, workspaces
    ctx.price_american_bounds_heston(ph)
    gs, hs = [], []
    for _ in range(reps):  # alternated: both see the same clocks and neighbours
        gs.append(ctx.price_american_bounds(pg))
        hs.append(ctx.price_american_bounds_heston(ph))

    def side(rs):
        med = lambda k: st.median(r[k] for r in rs)  # noqa: E731
        r0 = rs[0]
        return dict(ms=dict(fit=med("ms_fit"), lower=med("ms_lower"), upper=med("ms_upper"), total=med("ms_total")),
                    inner_path_steps=r0["inner_path_steps"],
                    inner_path_steps_per_s=r0["inner_path_steps"] / (med("ms_upper") * 1e-3),
                    lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"],
                    ci=[r0["ci_lo"], r0["ci_hi"]], gap=r0["upper"] - r0["lower"],
                    gap_rel=(r0["upper"] - r0["lower"]) / r0["lower"], n_exercised_lower=r0["n_exercised_lower"])

    g, h = side(gs), side(hs)
    eu = ctx.price_european(_ffi.make_params(model="heston", heston_scheme=scheme, is_put=True, n_paths=4_000_000,
                                             n_steps=N, seed=42, **HP))
    flows = {}
    for sem in ("reference", "two_pass", "textbook"):
        q = _ffi.make_params(model="heston", heston_scheme=scheme, semantics=sem, is_put=True, n_paths=1_000_000,
                             n_steps=N, seed=42, **HP)
        flows[sem] = ctx.price_american(q)["price"]
    out = dict(N=N, reps=reps, scheme=scheme, n_lower=hs[0]["n_lower"], n_outer=hs[0]["n_outer"], n_inner=hs[0]["n_inner"],
               heston=h, gbm=g, ratio_upper=h["ms"]["upper"] / g["ms"]["upper"], ratio_total=h["ms"]["total"] / g["ms"]["total"],
               ratio_per_inner_step=g["inner_path_steps_per_s"] / h["inner_path_steps_per_s"],
               european_put=eu["price"], in_sample_flows=flows)
    rows.append(out)
    print(json.dumps(out), flush=True)

o = [f"tools/time_heston_bounds.py {reps} on one MI355X: the ATM put (S0 = K = 100, r = 0.05, T = 1, N = {N}; textbook policy fitted on "
     "100,000 paths),",
     f"default sizes (n_lower 1M, n_outer 8192, n_inner 1024), HIP-event medians of {reps} in ms.  Two calls alternate in one process:",
     "  heston   omc_price_american_bounds_heston, v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7, the scheme of the row",
     "  gbm      omc_price_american_bounds, sigma = 0.2 (the parent's kernels: the yardstick)", "",
     "  scheme           call       fit    lower    upper    total   inner path-steps  path-steps/s   bracket"
     "                               gap    gap / lower"]
for r in rows:
    for k in ("heston", "gbm"):
        s, m = r[k], r[k]["ms"]
        o.append(f"  {r['scheme']:<16s} {k:<7s} {m['fit']:7.3f} {m['lower']:8.4f} {m['upper']:8.3f} {m['total']:8.3f} "
                 f"{s['inner_path_steps']:18d} {s['inner_path_steps_per_s']:13.3e}   [{s['lower']:.4f} ({s['se_lower']:.4f}), "
                 f"{s['upper']:.4f} ({s['se_upper']:.4f})]  {s['gap']:.4f}  {100 * s['gap_rel']:.2f} %")
o += ["", "  scheme           total heston/gbm  upper heston/gbm  time per inner path-step heston/gbm  European put (4M paths)  "
      "in-sample reference / two_pass / textbook (1M paths)"]
for r in rows:
    f = r["in_sample_flows"]
    o.append(f"  {r['scheme']:<16s} {r['ratio_total']:16.3f} {r['ratio_upper']:17.3f} {r['ratio_per_inner_step']:35.3f} "
             f"{r['european_put']:24.4f}  {f['reference']:.4f} / {f['two_pass']:.4f} / {f['textbook']:.4f}")
o += ["", "The raw lines:"] + [json.dumps(r) for r in rows]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(o) + "\n")

"""HIP-event cost and bracket of omc_price_american_bounds_barrier at the default sizes (textbook
policy fitted on 100,000 paths; n_lower 1M, n_outer 8192, n_inner 1024; S0 = K = 100, r = 0.05, T = 1, N = 50): the
down-and-out ATM put with H = 90 under GBM (sigma = 0.2) and under Heston (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7,
the reference scheme).
Three calls alternate in one process, so all see the same clocks and neighbours, and the times are medians of the calls' own
HIP events:
  plain      omc_price_american_bounds / omc_price_american_bounds_heston on the same config: the kernels the barrier law
             wraps (the yardstick)
  far        the barrier call with a barrier no path reaches (H = 0.001): the knock state and the list-driven sweep with
             every item kept, nothing saved -- its results carry plain's bits
  barrier    the barrier call with H = 90
The share of inner path-steps saved by stopping at the hit: the barrier call's steps against those of `nostop`, the vanilla
call run with the barrier call's policy as a given table -- the same exercise decisions where the option is live, no knock
stop, no dead items.
And the bracket beside the quote of price_barrier_option (omc_price_barrier, two-pass flow, 1M paths).
Prints one JSON line per row and writes a table of them and the lines to profiles/barrier_bounds_time.txt (or the path given).
usage: time_barrier_bounds.py [reps] [out_path]"""
import json
import os
import statistics as st
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "barrier_bounds_time.txt")
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
T, N, H, KIND = 1.0, 50, 90.0, "down-and-out"
ctx = _ffi.default_context(0)


def params(model, n_paths):
    if model == "gbm":
        return _ffi.make_params(semantics="two_pass", is_put=True, n_paths=n_paths, n_steps=N, T=T, seed=42)
    return _ffi.make_params(model="heston", heston_scheme="reference", semantics="two_pass", is_put=True, n_paths=n_paths,
                            n_steps=N, T=T, seed=42, **HP)


def side(rs):
    med = lambda k: st.median(r[k] for r in rs)  # noqa: E731
    r0 = rs[0]
    return dict(ms=dict(fit=med("ms_fit"), lower=med("ms_lower"), upper=med("ms_upper"), total=med("ms_total")),
                inner_path_steps=r0["inner_path_steps"], ns_per_kilostep=med("ms_upper") * 1e9 / max(r0["inner_path_steps"], 1),
                lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"])


rows = []
for model in ("gbm", "heston"):
    plain = ctx.price_american_bounds if model == "gbm" else ctx.price_american_bounds_heston
    p = params(model, 100_000)
    calls = dict(plain=lambda: plain(p), far=lambda: ctx.price_barrier_bounds(p, KIND, 1e-3),
                 barrier=lambda: ctx.price_barrier_bounds(p, KIND, H))
    got = {k: [] for k in calls}
    for f in calls.values():  # warm-up: code objects, workspaces
        f()
    for _ in range(reps):  # alternated
        for k, f in calls.items():
            got[k].append(f())
    s = {k: side(v) for k, v in got.items()}
    same = all(got["far"][0][k] == got["plain"][0][k] for k in ("lower", "upper", "se_lower", "se_upper", "inner_path_steps"))
    nostop = plain(p, policy="given", betas=got["barrier"][0]["betas"])
    quote = ctx.price_barrier(params(model, 1_000_000), KIND, H)
    out = dict(model=model, N=N, H=H, kind=KIND, reps=reps, **s, far_has_plain_bits=same,
               ratio_upper_far=s["far"]["ms"]["upper"] / s["plain"]["ms"]["upper"],
               ratio_total_far=s["far"]["ms"]["total"] / s["plain"]["ms"]["total"],
               ratio_upper_barrier=s["barrier"]["ms"]["upper"] / s["plain"]["ms"]["upper"],
               ratio_total_barrier=s["barrier"]["ms"]["total"] / s["plain"]["ms"]["total"],
               ratio_per_step_barrier=s["barrier"]["ns_per_kilostep"] / s["plain"]["ns_per_kilostep"],
               nostop_inner_path_steps=nostop["inner_path_steps"],
               steps_saved=1.0 - s["barrier"]["inner_path_steps"] / nostop["inner_path_steps"],
               quote=quote["price"], quote_se=(max(quote["sumsq"] / 1e6 - quote["price"] ** 2, 0.0) / 1e6) ** 0.5,
               euro_out=quote["euro_out"], hit_prob=quote["hit_prob"],
               ci=[got["barrier"][0]["ci_lo"], got["barrier"][0]["ci_hi"]])
    rows.append(out)
    print(json.dumps(out), flush=True)

o = [f"tools/time_barrier_bounds.py {reps} on one MI355X: S0 = K = 100, r = 0.05, T = 1, N = 50; the American down-and-out put, H = 90,",
     "discrete monitoring; textbook policy fitted on 100,000 paths, default sizes (n_lower 1M, n_outer 8192, n_inner 1024),",
     f"HIP-event medians of {reps} in ms.  Three calls alternate in one process:",
     "  plain    gbm: omc_price_american_bounds, sigma = 0.2; heston: omc_price_american_bounds_heston, v0 = theta = 0.04, kappa = 2,",
     "           xi = 0.3, rho = -0.7, reference scheme (the kernels the barrier law wraps: the yardstick)",
     "  far      omc_price_american_bounds_barrier with H = 0.001: the knock state and the list-driven sweep, nothing saved",
     "  barrier  omc_price_american_bounds_barrier with H = 90", "",
     "  model   call        fit    lower    upper    total   inner path-steps  ns / 1000 steps   bracket"]
for r in rows:
    for k in ("plain", "far", "barrier"):
        s, m = r[k], r[k]["ms"]
        o.append(f"  {r['model']:<7s} {k:<8s} {m['fit']:7.3f} {m['lower']:8.4f} {m['upper']:8.3f} {m['total']:8.3f} "
                 f"{s['inner_path_steps']:18d} {s['ns_per_kilostep']:16.4f}   [{s['lower']:.4f} ({s['se_lower']:.4f}), "
                 f"{s['upper']:.4f} ({s['se_upper']:.4f})]")
o += ["", "  model    upper far/plain  total far/plain  upper barrier/plain  total barrier/plain  per inner step barrier/plain  "
      "far has plain's bits"]
for r in rows:
    o.append(f"  {r['model']:<7s} {r['ratio_upper_far']:16.3f} {r['ratio_total_far']:16.3f} {r['ratio_upper_barrier']:20.3f} "
             f"{r['ratio_total_barrier']:20.3f} {r['ratio_per_step_barrier']:29.3f}  {r['far_has_plain_bits']}")
o += ["", "Inner path-steps saved by stopping at the hit (and by never starting a dead item): the barrier call's steps against the",
      "vanilla call's with the barrier call's policy given (the same exercise decisions where the option is live)",
      "  model    barrier steps        without the stop    saved"]
for r in rows:
    o.append(f"  {r['model']:<7s} {r['barrier']['inner_path_steps']:14d} {r['nostop_inner_path_steps']:22d} {100 * r['steps_saved']:8.1f} %")
o += ["", "The bracket beside the quote: quote = omc_price_barrier (two-pass flow) on 1M paths; european = its euro_out on the same paths",
      "  model     quote (se)          lower (se)          upper (se)          95 % interval          european   paths hit"]
for r in rows:
    b = r["barrier"]
    o.append(f"  {r['model']:<7s} {r['quote']:.4f} ({r['quote_se']:.4f})   {b['lower']:.4f} ({b['se_lower']:.4f})   "
             f"{b['upper']:.4f} ({b['se_upper']:.4f})   [{r['ci'][0]:.4f}, {r['ci'][1]:.4f}]   {r['euro_out']:.4f}   "
             f"{100 * r['hit_prob']:.1f} %")
o += ["", "The raw lines:"] + [json.dumps(r) for r in rows]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(o) + "\n")

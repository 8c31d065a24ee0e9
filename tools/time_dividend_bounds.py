"""HIP-event cost and bracket of omc_price_american_bounds_div at the default sizes (textbook policy
fitted on 100,000 paths; n_lower 1M, n_outer 8192, n_inner 1024; S0 = K = 100, r = 0.05, T = 1), under GBM (sigma = 0.2) and
under Heston (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7, the reference scheme), in three forms:
  dates50    the ATM put at N = 50, every date
  monthly    N = 252 with exercise_every = 21
  checked    N = 50 with the payoff check
Three calls alternate in one process, so all see the same clocks and neighbours, and the times are medians of the calls' own
HIP events:
  plain      omc_price_american_bounds / omc_price_american_bounds_heston: the kernels the dividend law wraps (the yardstick)
  nodiv      the dividend call with n_div = 0: the date test alone -- the countdown, the ballot and the branch, never taken
  div        the dividend call with four quarterly cash dividends of 1.0: the date test and the hit path
And the bracket for the quote of price_american_dividends: the call at N = 252 with quarterly cash dividends of 1.0, next to
omc_price_american_div's two-pass quote on 1M paths.
Prints one JSON line per row and writes a table of them and the lines to profiles/dividend_bounds_time.txt (or the path given).
usage: time_dividend_bounds.py [reps] [out_path]"""
import json
import os
import statistics as st
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "dividend_bounds_time.txt")
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
T = 1.0
DIVS = [(0.125 + 0.25 * i, 1.0, "cash") for i in range(4)]
ctx = _ffi.default_context(0)


def params(model, N, n_paths, is_put=True):
    if model == "gbm":
        return _ffi.make_params(semantics="two_pass", is_put=is_put, n_paths=n_paths, n_steps=N, T=T, seed=42)
    return _ffi.make_params(model="heston", heston_scheme="reference", semantics="two_pass", is_put=is_put, n_paths=n_paths,
                            n_steps=N, T=T, seed=42, **HP)


def side(rs):
    med = lambda k: st.median(r[k] for r in rs)  # noqa: E731
    r0 = rs[0]
    return dict(ms=dict(fit=med("ms_fit"), lower=med("ms_lower"), upper=med("ms_upper"), total=med("ms_total")),
                inner_path_steps=r0["inner_path_steps"], ns_per_kilostep=med("ms_upper") * 1e9 / max(r0["inner_path_steps"], 1),
                lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"])


FORMS = (("dates50", 50, {}), ("monthly", 252, dict(exercise_every=21)), ("checked", 50, dict(suboptimality_check="payoff")))
rows = []
for model in ("gbm", "heston"):
    plain = ctx.price_american_bounds if model == "gbm" else ctx.price_american_bounds_heston
    for form, N, kw in FORMS:
        p = params(model, N, 100_000)
        calls = dict(plain=lambda: plain(p, **kw), nodiv=lambda: ctx.price_american_bounds_div(p, 0.0, (), **kw),
                     div=lambda: ctx.price_american_bounds_div(p, 0.0, DIVS, **kw))
        got = {k: [] for k in calls}
        for f in calls.values():  # warm-up: code objects, workspaces
            f()
        for _ in range(reps):  # alternated
            for k, f in calls.items():
                got[k].append(f())
        s = {k: side(v) for k, v in got.items()}
        same = all(got["nodiv"][0][k] == got["plain"][0][k] for k in ("lower", "upper", "se_lower", "se_upper", "inner_path_steps"))
        out = dict(model=model, form=form, N=N, reps=reps, **s, nodiv_has_plain_bits=same,
                   ratio_upper_nodiv=s["nodiv"]["ms"]["upper"] / s["plain"]["ms"]["upper"],
                   ratio_upper_div=s["div"]["ms"]["upper"] / s["plain"]["ms"]["upper"],
                   ratio_total_nodiv=s["nodiv"]["ms"]["total"] / s["plain"]["ms"]["total"],
                   ratio_total_div=s["div"]["ms"]["total"] / s["plain"]["ms"]["total"],
                   ratio_per_step_nodiv=s["nodiv"]["ns_per_kilostep"] / s["plain"]["ns_per_kilostep"],
                   ratio_per_step_div=s["div"]["ns_per_kilostep"] / s["plain"]["ns_per_kilostep"])
        rows.append(out)
        print(json.dumps(out), flush=True)

# the bracket for the dividend quote: a call, N = 252, quarterly cash dividends of 1.0
quotes = []
for model in ("gbm", "heston"):
    b = ctx.price_american_bounds_div(params(model, 252, 100_000, is_put=False), 0.0, DIVS)
    q = ctx.price_american_div(params(model, 252, 1_000_000, is_put=False), 0.0, DIVS)
    e = ctx.price_american_bounds_div(params(model, 252, 100_000, is_put=False), 0.0, DIVS, policy="given",
                                      betas=[[0.0] * 4] * 253, n_outer=2, n_inner=2)  # never exercising: the European value
    out = dict(model=model, N=252, quote=q["price"], quote_se=(max(q["sumsq"] / 1e6 - q["price"] ** 2, 0.0) / 1e6) ** 0.5,
               lower=b["lower"], se_lower=b["se_lower"], upper=b["upper"], se_upper=b["se_upper"], ci=[b["ci_lo"], b["ci_hi"]],
               european=e["lower"], se_european=e["se_lower"], ms_total=b["ms_total"], inner_path_steps=b["inner_path_steps"])
    quotes.append(out)
    print(json.dumps(out), flush=True)

o = [f"tools/time_dividend_bounds.py {reps} on one MI355X: S0 = K = 100, r = 0.05, T = 1; textbook policy fitted on 100,000 paths,",
     f"default sizes (n_lower 1M, n_outer 8192, n_inner 1024), HIP-event medians of {reps} in ms.  Three calls alternate in one process:",
     "  plain  gbm: omc_price_american_bounds, sigma = 0.2; heston: omc_price_american_bounds_heston, v0 = theta = 0.04, kappa = 2,",
     "         xi = 0.3, rho = -0.7, reference scheme (the kernels the dividend law wraps: the yardstick)",
     "  nodiv  omc_price_american_bounds_div with n_div = 0: the date test alone (its results carry plain's bits)",
     "  div    omc_price_american_bounds_div with cash dividends of 1.0 at t = 0.125, 0.375, 0.625, 0.875",
     "forms: dates50 = the put at N = 50; monthly = N = 252, exercise_every = 21; checked = N = 50 with the payoff check", "",
     "  model   form     call       fit    lower    upper    total   inner path-steps  ns / 1000 steps   bracket"]
for r in rows:
    for k in ("plain", "nodiv", "div"):
        s, m = r[k], r[k]["ms"]
        o.append(f"  {r['model']:<7s} {r['form']:<8s} {k:<6s} {m['fit']:7.3f} {m['lower']:8.4f} {m['upper']:8.3f} {m['total']:8.3f} "
                 f"{s['inner_path_steps']:18d} {s['ns_per_kilostep']:16.4f}   [{s['lower']:.4f} ({s['se_lower']:.4f}), "
                 f"{s['upper']:.4f} ({s['se_upper']:.4f})]")
o += ["", "  model   form      upper nodiv/plain  upper div/plain  total nodiv/plain  total div/plain  per inner step nodiv/plain  "
      "per inner step div/plain  nodiv has plain's bits"]
for r in rows:
    o.append(f"  {r['model']:<7s} {r['form']:<8s} {r['ratio_upper_nodiv']:18.3f} {r['ratio_upper_div']:16.3f} "
             f"{r['ratio_total_nodiv']:18.3f} {r['ratio_total_div']:16.3f} {r['ratio_per_step_nodiv']:27.3f} "
             f"{r['ratio_per_step_div']:25.3f}  {r['nodiv_has_plain_bits']}")
o += ["", "The bracket for the dividend quote: the call at N = 252 with the four cash dividends of 1.0 (default sizes); quote ="
      " omc_price_american_div on 1M paths;", "european = the never-exercising policy's lower bound (1M paths)",
      "  model     quote (se)          lower (se)          upper (se)          95 % interval          european (se)"]
for r in quotes:
    o.append(f"  {r['model']:<7s} {r['quote']:.4f} ({r['quote_se']:.4f})   {r['lower']:.4f} ({r['se_lower']:.4f})   "
             f"{r['upper']:.4f} ({r['se_upper']:.4f})   [{r['ci'][0]:.4f}, {r['ci'][1]:.4f}]   {r['european']:.4f} "
             f"({r['se_european']:.4f})")
o += ["", "The raw lines:"] + [json.dumps(r) for r in rows + quotes]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(o) + "\n")

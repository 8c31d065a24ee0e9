"""HIP-event cost and bracket of omc_price_american_bounds_jump for the ATM put (S0 = K = 100, r = 0.05, T = 1; jumps J ~
N(-0.1, 0.15^2); textbook policy fitted on 100,000 paths; default sizes n_lower 1M, n_outer 8192, n_inner 1024) at N = 50, under
Merton (GBM, sigma = 0.2) and under Bates (Heston, v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7, the reference scheme), each
at one jump a year and at lambda T / N = 0.5 (where nearly every wave has a jumping lane at every step, so the ballot rarely
saves anything), next to the jump-free call of the same model -- omc_price_american_bounds / omc_price_american_bounds_heston
-- at the same sizes in the same process: the calls alternate, the times are medians of the calls' own HIP events.  Prints
one JSON line per (model, lambda) -- the times of both, the ratio of the upper phases and of the totals, inner path-steps per
second of both, both brackets, and the quote of omc_price_american_jump (1M paths) that the jump bracket belongs to -- and
writes a table of them and the lines to profiles/jump_bounds_time.txt (or the path given).
usage: time_jump_bounds.py [reps] [out_path] [N]"""
import json
import os
import statistics as st
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "jump_bounds_time.txt")
N = int(sys.argv[3]) if len(sys.argv) > 3 else 50
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
MU, SJ, T = -0.1, 0.15, 1.0
ctx = _ffi.default_context(0)


def params(model, n_paths):
    if model == "merton":
        return _ffi.make_params(semantics="two_pass", is_put=True, n_paths=n_paths, n_steps=N, T=T, seed=42)
    return _ffi.make_params(model="heston", heston_scheme="reference", semantics="two_pass", is_put=True, n_paths=n_paths,
                            n_steps=N, T=T, seed=42, **HP)


def side(rs):
    med = lambda k: st.median(r[k] for r in rs)  # noqa: E731
    r0 = rs[0]
    return dict(ms=dict(fit=med("ms_fit"), lower=med("ms_lower"), upper=med("ms_upper"), total=med("ms_total")),
                inner_path_steps=r0["inner_path_steps"], inner_path_steps_per_s=r0["inner_path_steps"] / (med("ms_upper") * 1e-3),
                lower=r0["lower"], se_lower=r0["se_lower"], upper=r0["upper"], se_upper=r0["se_upper"],
                ci=[r0["ci_lo"], r0["ci_hi"]], gap=r0["upper"] - r0["lower"], n_exercised_lower=r0["n_exercised_lower"])


rows = []
for model in ("merton", "bates"):
    plain = ctx.price_american_bounds if model == "merton" else ctx.price_american_bounds_heston
    for lam in (1.0, 0.5 * N / T):
        p = params(model, 100_000)
        jump = (lam, MU, SJ)
        plain(p)  # warm-up: code objects, workspaces
        ctx.price_american_bounds_jump(p, jump, 0.0)
        vs, js = [], []
        for _ in range(reps):  # alternated: both see the same clocks and neighbours
            vs.append(plain(p))
            js.append(ctx.price_american_bounds_jump(p, jump, 0.0))
        v, j = side(vs), side(js)
        quote = ctx.price_american_jump(params(model, 1_000_000), jump, 0.0)
        out = dict(N=N, reps=reps, model=model, jump_intensity=lam, x=lam * T / N, jump_mean=MU, jump_vol=SJ,
                   n_lower=js[0]["n_lower"], n_outer=js[0]["n_outer"], n_inner=js[0]["n_inner"], jump=j, jump_free=v,
                   ratio_upper=j["ms"]["upper"] / v["ms"]["upper"], ratio_total=j["ms"]["total"] / v["ms"]["total"],
                   ratio_per_inner_step=v["inner_path_steps_per_s"] / j["inner_path_steps_per_s"],
                   two_pass_quote=quote["price"])
        rows.append(out)
        print(json.dumps(out), flush=True)

o = [f"tools/time_jump_bounds.py {reps} on one MI355X: the ATM put (S0 = K = 100, r = 0.05, T = 1, N = {N}; textbook policy fitted on "
     "100,000 paths),",
     f"default sizes (n_lower 1M, n_outer 8192, n_inner 1024), HIP-event medians of {reps} in ms.  Two calls alternate in one process:",
     "  jump       omc_price_american_bounds_jump, J ~ N(-0.1, 0.15^2), q = 0, lambda of the row (x = lambda T / N)",
     "  jump-free  merton: omc_price_american_bounds, sigma = 0.2; bates: omc_price_american_bounds_heston, v0 = theta = 0.04,",
     "             kappa = 2, xi = 0.3, rho = -0.7, reference scheme (the parent's kernels: the yardstick)", "",
     "  model   lambda     x  call           fit    lower    upper    total   inner path-steps  path-steps/s   bracket"
     "                               gap"]
for r in rows:
    for k, name in (("jump", "jump"), ("jump_free", "jump-free")):
        s, m = r[k], r[k]["ms"]
        o.append(f"  {r['model']:<7s} {r['jump_intensity']:6.2f} {r['x']:5.2f}  {name:<10s} {m['fit']:7.3f} {m['lower']:8.4f} "
                 f"{m['upper']:8.3f} {m['total']:8.3f} {s['inner_path_steps']:18d} {s['inner_path_steps_per_s']:13.3e}   "
                 f"[{s['lower']:.4f} ({s['se_lower']:.4f}), {s['upper']:.4f} ({s['se_upper']:.4f})]  {s['gap']:.4f}")
o += ["", "  model   lambda     x  total jump/jump-free  upper jump/jump-free  time per inner path-step jump/jump-free  "
      "two-pass quote of omc_price_american_jump (1M paths)"]
for r in rows:
    o.append(f"  {r['model']:<7s} {r['jump_intensity']:6.2f} {r['x']:5.2f} {r['ratio_total']:21.3f} {r['ratio_upper']:21.3f} "
             f"{r['ratio_per_inner_step']:39.3f}  {r['two_pass_quote']:.4f}")
o += ["", "The raw lines:"] + [json.dumps(r) for r in rows]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(o) + "\n")

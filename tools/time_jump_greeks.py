"""Cost of omc_price_american_jump_greeks next to the pricing it hedges: the ATM put on 1M paths x 252
steps with lambda = 1 jump a year, J ~ N(-0.1, 0.15^2) (S0 = K = 100, r = 0.05, T = 1), under GBM (Merton, sigma = 0.2) and
under Heston (Bates: v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7, the reference scheme).  Two calls alternate in one
process, so both see the same clocks and neighbours:
  price    omc_price_american_jump: generator, pass 1, pass 2
  greeks   omc_price_american_jump_greeks: generator, pass 1, the sweep on regenerated paths
Reported: the whole call (wall clock around it) and the calls' own HIP-event times, medians of the repetitions, and the
ratios ms_greeks / ms_jump_paths (the sweep redoes the generator's arithmetic on three scenarios with the running sums, and
stores nothing), ms_greeks / ms_pass2 (what it replaces) and whole call / whole call.
Prints one JSON line per model and writes a table and the lines to profiles/jump_greeks_time.txt (or the path given).
usage: time_jump_greeks.py [reps] [out_path]"""
import json
import os
import statistics as st
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "jump_greeks_time.txt")
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
M, N, T = 1_000_000, 252, 1.0
JUMP = (1.0, -0.1, 0.15)
ctx = _ffi.default_context(0)


def params(model):
    if model == "gbm":
        return _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, T=T, seed=42)
    return _ffi.make_params(model="heston", heston_scheme="reference", semantics="two_pass", is_put=True, n_paths=M, n_steps=N,
                            T=T, seed=42, **HP)


def timed(f):
    ctx.sync()
    t0 = time.perf_counter()
    r = f()
    return dict(r, wall_ms=(time.perf_counter() - t0) * 1e3)


rows = []
for model in ("gbm", "heston"):
    p = params(model)
    calls = dict(price=lambda: ctx.price_american_jump(p, JUMP, 0.0), greeks=lambda: ctx.price_american_jump_greeks(p, JUMP, 0.0))
    got = {k: [] for k in calls}
    for f in calls.values():  # warm-up: code objects, workspaces
        f()
    for _ in range(reps):  # alternated
        for k, f in calls.items():
            got[k].append(timed(f))
    med = lambda k, key: st.median(r[key] for r in got[k])  # noqa: E731
    pr, gk = got["price"][0], got["greeks"][0]
    out = dict(model=model, n_paths=M, n_steps=N, reps=reps,
               price=dict(wall_ms=med("price", "wall_ms"), ms_jump_paths=med("price", "ms_jump_paths"), ms_pass1=med("price", "ms_pass1"),
                          ms_pass2=med("price", "ms_pass2"), ms_total=med("price", "ms_total"), price=pr["price"],
                          n_exercised=pr["n_exercised"]),
               greeks=dict(wall_ms=med("greeks", "wall_ms"), ms_paths=med("greeks", "ms_paths"), ms_pass1=med("greeks", "ms_pass1"),
                           ms_greeks=med("greeks", "ms_greeks"), ms_total=med("greeks", "ms_total"), price=gk["price"],
                           n_exercised=gk["n_exercised"],
                           **{k: gk[k] for k in ("delta", "se_delta", "gamma", "se_gamma", "vega", "se_vega", "rho", "se_rho", "theta",
                                                 "se_theta", "epsilon", "se_epsilon", "dlambda", "se_dlambda", "dmu_j", "se_dmu_j",
                                                 "dsigma_j", "se_dsigma_j", "theta_score", "se_theta_score", "n_jumps")}))
    out["same_counts"] = pr["n_exercised"] == gk["n_exercised"] and pr["n_zero"] == gk["n_zero"] and pr["sum_nitm"] == gk["sum_nitm"]
    out["ratio_greeks_to_jump_paths"] = out["greeks"]["ms_greeks"] / out["price"]["ms_jump_paths"]
    out["ratio_greeks_to_pass2"] = out["greeks"]["ms_greeks"] / out["price"]["ms_pass2"]
    out["ratio_call_events"] = out["greeks"]["ms_total"] / out["price"]["ms_total"]
    out["ratio_call_wall"] = out["greeks"]["wall_ms"] / out["price"]["wall_ms"]
    rows.append(out)
    print(json.dumps(out), flush=True)

o = [f"tools/time_jump_greeks.py {reps} on one MI355X: the ATM put, S0 = K = 100, r = 0.05, T = 1, {M} paths x {N} steps, lambda = 1,",
     "J ~ N(-0.1, 0.15^2); gbm: sigma = 0.2; heston: v0 = theta = 0.04, kappa = 2, xi = 0.3,",
     f"rho = -0.7, reference scheme.  Medians of {reps} alternated calls in ms: wall = the whole call, the others HIP events.", "",
     "  model   call     wall    paths    pass1    pass2   greeks   events total"]
for r in rows:
    a, b = r["price"], r["greeks"]
    o.append(f"  {r['model']:<7s} price  {a['wall_ms']:8.3f} {a['ms_jump_paths']:8.3f} {a['ms_pass1']:8.3f} {a['ms_pass2']:8.3f} {'-':>8s} "
             f"{a['ms_total']:8.3f}")
    o.append(f"  {r['model']:<7s} greeks {b['wall_ms']:8.3f} {b['ms_paths']:8.3f} {b['ms_pass1']:8.3f} {'-':>8s} {b['ms_greeks']:8.3f} "
             f"{b['ms_total']:8.3f}")
o += ["", "  model   ms_greeks / ms_jump_paths   ms_greeks / ms_pass2   call / call (events)   call / call (wall)   same counts"]
for r in rows:
    o.append(f"  {r['model']:<7s} {r['ratio_greeks_to_jump_paths']:24.3f} {r['ratio_greeks_to_pass2']:22.3f} {r['ratio_call_events']:22.3f} "
             f"{r['ratio_call_wall']:20.3f}   {r['same_counts']}")
o += ["", "  model   price        delta (se)            gamma (se)            vega (se)            rho (se)             theta (se)"
      "           epsilon (se)          dlambda (se)          dmu_j (se)            dsigma_j (se)"]
for r in rows:
    g = r["greeks"]
    o.append(f"  {r['model']:<7s} {g['price']:.5f}  " + "  ".join(f"{g[k]:+.5f} ({g['se_' + k]:.5f})" for k in
                                                                  ("delta", "gamma", "vega", "rho", "theta", "epsilon", "dlambda", "dmu_j",
                                                                   "dsigma_j")))
o += ["", "The raw lines:"] + [json.dumps(r) for r in rows]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(o) + "\n")

"""HIP-event cost of omc_price_american_chain_bounds against the same quotes as single calls, at the
README's bounds configuration: S0 = 100, r = 0.05, sigma = 0.2, T = 1, 50 dates, the textbook policy fitted on 100,000 paths,
default sizes (n_lower 1M, n_outer 8192, n_inner 1024).
  chain8     8 puts at strikes 80 .. 120 in one call, against the 8 omc_price_american_bounds calls
  chain4     the 4 strikes 90, 100, 110, 120;  chain2: 95 and 105
  heston8    the 8 puts under Heston (v0 = theta = 0.04, kappa = 2, xi = 0.3, rho = -0.7, the reference scheme), against the 8
             omc_price_american_bounds_heston calls
The chain and its single calls alternate in one process, so both see the same clocks and neighbours; the times are the calls'
own HIP events (ms_total; the single side is the sum over its calls), reported as median, minimum and maximum of the
repetitions.  `spread` is the larger of the two sides' (maximum - minimum): the chain is faster only where the medians differ
by more than it.  Also: the steps the chain simulated against the sum of the entries' own inner path steps, and the worst
deviation of an entry from its single call.
Prints one JSON line per row and writes a table of them and the lines to profiles/chain_bounds_time.txt (or the path given).
usage: time_chain_bounds.py [reps] [out_path]
       time_chain_bounds.py --deviation     the worst deviations over the tests' tolerance cases (tests/helpers), no timing"""
import json
import os
import statistics as st
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from options_model_amd import _ffi  # noqa: E402

HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
ctx = _ffi.default_context(0)


def deviation_report():
    """each entry of the tests' tolerance cases (and of the fuzz cases with refills) against its own single call"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import chain_bounds_case as cc
    from helpers import chain_bounds_catalogue as cat

    cases = dict(cat.TOLERANCE_CASES)
    scale = float(os.environ.get("OMC_FUZZ_SCALE", "1"))
    for c in cc.fuzz_cases(max(1, int(round(10 * scale)))):
        if c["n_inner"] > cc.EXACT_INNER:
            cases["fuzz-" + cc.case_id(c)] = c
    worst_up = worst_q = 0.0
    for name, case in cases.items():
        outs, info = cc.run_chain(ctx, case)
        ups, qs = zip(*(cc.deviation(o, cc.run_single(ctx, case, e)) for e, o in enumerate(outs)))
        worst_up, worst_q = max(worst_up, *ups), max(worst_q, *qs)
        print(json.dumps(dict(case=name, upper_rel=max(ups), q_rel=max(qs))), flush=True)
    print(json.dumps(dict(worst_upper_rel=worst_up, worst_q_rel=worst_q, cases=len(cases))), flush=True)


if "--deviation" in sys.argv:
    deviation_report()
    sys.exit(0)

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "chain_bounds_time.txt")
STRIKES8 = [80.0 + 40.0 * i / 7.0 for i in range(8)]
ROWS = (("chain8", "gbm", STRIKES8), ("chain4", "gbm", [90.0, 100.0, 110.0, 120.0]), ("chain2", "gbm", [95.0, 105.0]),
        ("heston8", "heston", STRIKES8))


def params(model, K):
    kw = dict(semantics="two_pass", is_put=True, n_paths=100_000, n_steps=50, S0=100.0, K=K, r=0.05, T=1.0, seed=42)
    if model == "gbm":
        return _ffi.make_params(sigma=0.2, **kw)
    return _ffi.make_params(model="heston", heston_scheme="reference", **kw, **HP)


def stats(xs):
    return dict(median=st.median(xs), min=min(xs), max=max(xs))


rows = []
for name, model, strikes in ROWS:
    single = ctx.price_american_bounds if model == "gbm" else ctx.price_american_bounds_heston
    chain = lambda: ctx.price_american_chain_bounds(params(model, strikes[0]), strikes, True)  # noqa: E731
    singles = lambda: [single(params(model, K)) for K in strikes]  # noqa: E731
    outs, info = chain()  # warm-up: code objects, workspaces
    ones = singles()
    t_chain, t_single, phases = [], [], []
    for _ in range(reps):  # alternated
        outs, info = chain()
        t_chain.append(info["ms_total"])
        phases.append(info)
        ones = singles()
        t_single.append(sum(o["ms_total"] for o in ones))
    c, s = stats(t_chain), stats(t_single)
    spread = max(c["max"] - c["min"], s["max"] - s["min"])
    own = [o["inner_path_steps"] for o in ones]
    exact = all(o[k] == r[k] for o, r in zip(outs, ones) for k in ("lower", "se_lower", "n_exercised_lower", "inner_path_steps"))
    out = dict(row=name, model=model, entries=len(strikes), reps=reps, chain_ms=c, singles_ms=s, spread_ms=spread,
               speedup=s["median"] / c["median"], faster_beyond_spread=bool(s["median"] - c["median"] > spread),
               chain_phases_ms={k: st.median(p[k] for p in phases) for k in ("ms_fit", "ms_lower", "ms_upper")},
               singles_phases_ms={k: sum(o[k] for o in ones) for k in ("ms_fit", "ms_lower", "ms_upper")},
               n_groups=info["n_groups"], steps_simulated=info["inner_path_steps_simulated"], steps_entries_sum=sum(own),
               steps_entries_max=max(own), lower_bits_equal=exact,
               worst_upper_rel=max(abs(o["upper"] - r["upper"]) / r["upper"] for o, r in zip(outs, ones)),
               brackets=[[o["lower"], o["upper"]] for o in outs])
    rows.append(out)
    print(json.dumps(out), flush=True)

o = [f"tools/time_chain_bounds.py {reps} on one MI355X: S0 = 100, r = 0.05, sigma = 0.2, T = 1, 50 dates, puts; textbook policy fitted",
     f"on 100,000 paths, default sizes (n_lower 1M, n_outer 8192, n_inner 1024); HIP-event ms_total, median [min, max] of {reps}.",
     "chain = one omc_price_american_chain_bounds call; singles = the sum over the entries' own omc_price_american_bounds",
     "(heston8: omc_price_american_bounds_heston) calls; the two sides alternate in one process.  spread = the larger (max - min).",
     "",
     "  row      entries   chain ms               singles ms             spread  singles/chain  beyond spread   steps simulated / "
     "sum of entries' / max entry's"]
for r in rows:
    c, s = r["chain_ms"], r["singles_ms"]
    o.append(f"  {r['row']:<8s} {r['entries']:7d}   {c['median']:7.3f} [{c['min']:.3f}, {c['max']:.3f}]   {s['median']:7.3f} "
             f"[{s['min']:.3f}, {s['max']:.3f}]  {r['spread_ms']:6.3f}  {r['speedup']:13.2f}  {str(r['faster_beyond_spread']):<13s}   "
             f"{r['steps_simulated']} / {r['steps_entries_sum']} / {r['steps_entries_max']}")
o += ["", "  row      phase medians, chain (fit / lower / upper)     singles summed (fit / lower / upper)     worst |upper - single's| / upper"]
for r in rows:
    c, s = r["chain_phases_ms"], r["singles_phases_ms"]
    o.append(f"  {r['row']:<8s} {c['ms_fit']:8.3f} / {c['ms_lower']:.3f} / {c['ms_upper']:.3f}"
             f"                     {s['ms_fit']:8.3f} / {s['ms_lower']:.3f} / {s['ms_upper']:.3f}              {r['worst_upper_rel']:.2e}")
o += ["", "The raw lines:"] + [json.dumps(r) for r in rows]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(o) + "\n")

"""Cost of the Greeks of a whole option chain (omc_price_american_chain_greeks) against n omc_price_american_greeks calls.

Sizes: 1M paths x 252 steps and 131,072 x 50, GBM, S0 = 100, 8 puts at K = 80 .. 115 in steps of 5 and 16 at K = 80 .. 117.5 in
steps of 2.5; besides, one Heston size (131,072 x 50, 8 puts, scheme 1: full storage).  Per configuration, in ONE process,
alternating, medians of `reps` after `warm` warm-ups of the HIP-event time of the whole call (first launch to last completion):
    (a) the chain's Greeks, default block order (the entries of 8 neighbouring column blocks dispatched together)
    (b) the same with the other block order (entry slowest: n sweeps back to back in one grid)
    (c) "chain_greeks_k" = 1: one sweep launch per entry
    (d) the n single omc_price_american_greeks calls, summed
with the phases of (a) from its info and ms_paths of (d), the generator of one call.  --baseline runs (d) alone -- what a build of
the parent commit can run; with --root DIR it takes the package and the library under DIR (an unpacked tree of that commit with
its library built) and never builds.  Printed per configuration:
    (a) < (d)                                 -- the acceptance
    (a) <= (d) - 0.8 (n - 1) ms_paths         -- DESIGN.md 13.4's condition: the generators the chain no longer runs, less a fifth
At 1M x 252 a last configuration times one strike as three one-entry chains -- American, monthly (21), quarterly (63) -- for the
sweep's time against the share of rows it visits.
One JSON line per configuration, on stdout and appended to --out FILE; the committed record is profiles/chain_greeks_time.txt.
Every configuration runs in a child process of its own under a time limit, and the first one that fails or runs out of time ends
the run (nothing more is started on the GPU after a fault).
usage: time_chain_greeks.py [--baseline] [--root DIR] [--out FILE] [reps] [warm]"""
import json
import os
import statistics as st
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1_000_000, 252, 8, "gbm"), (1_000_000, 252, 16, "gbm"), (131_072, 50, 8, "gbm"), (131_072, 50, 16, "gbm"),
           (131_072, 50, 8, "heston"), (1_000_000, 252, 0, "schedules")]
HESTON = dict(model="heston", heston_scheme=1, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
LIMIT_S = 240


def strikes(n):
    return [80.0 + 40.0 / n * i for i in range(n)]  # 8: steps of 5; 16: steps of 2.5


def med(rs):
    out = {f: st.median(r[f] for r in rs) for f in rs[0]}
    out["min_total"] = min(r["total"] for r in rs)
    return out


def one(M, N, n, kind, reps, warm, baseline, root, out_file=None):
    sys.path.insert(0, root)
    from options_model_amd import _ffi
    if root != ROOT:
        _ffi.load_library(build_if_missing=False)
    ctx = _ffi.default_context(0)
    kw = HESTON if kind == "heston" else {}
    out = dict(build="baseline" if baseline else "chain_greeks", M=M, N=N, n=n, kind=kind, reps=reps, warm=warm)

    def mk(K):
        return _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, K=K, seed=42, **kw)

    def chain(ks, every, order=0, width=-1):
        ctx.set_option("chain_greeks_order", order)
        ctx.set_option("chain_greeks_k", width)
        outs, info = ctx.price_american_chain_greeks(mk(ks[0]), ks, True, bump=0.01, exercise_every=every)
        return dict(total=info["ms_total"], paths=info["ms_paths"], pass1=info["ms_pass1"], greeks=info["ms_greeks"],
                    launches=info["n_sweep_launches"], folded=info["folded"], delta0=outs[0]["delta"])

    def singles(ks):
        outs = [ctx.price_american_greeks(mk(K), bump=0.01) for K in ks]
        return dict(total=sum(o["ms_total"] for o in outs), paths=st.median(o["ms_paths"] for o in outs),
                    greeks=sum(o["ms_greeks"] for o in outs), pass1=sum(o["ms_pass1"] for o in outs), delta0=outs[0]["delta"])

    if kind == "schedules":
        runs = {name: (lambda k=k: chain([100.0], [k])) for name, k in (("american", 0), ("monthly", 21), ("quarterly", 63))}
    else:
        ks = strikes(n)
        runs = {"d_singles": lambda: singles(ks)}
        if not baseline:
            runs = {"a_chain": lambda: chain(ks, 0), "b_other_order": lambda: chain(ks, 0, order=1),
                    "c_one_per_launch": lambda: chain(ks, 0, width=1), **runs}
    samples = {k: [] for k in runs}
    for it in range(warm + reps):
        for k, fn in runs.items():  # alternating: every variant sees the same state of the machine
            r = fn()
            if it >= warm:
                samples[k].append(r)
    for k, rs in samples.items():
        out[k] = med(rs)
    if kind == "schedules":
        rows = {"american": N - 1, "monthly": (N - 1) // 21, "quarterly": (N - 1) // 63}
        out["greeks_vs_rows"] = {k: dict(greeks_ratio=out[k]["greeks"] / out["american"]["greeks"], rows_ratio=(rows[k] + 1) / N)
                                 for k in rows}
    elif not baseline:
        a, b, c, d = (out[k]["total"] for k in ("a_chain", "b_other_order", "c_one_per_launch", "d_singles"))
        bound = d - 0.8 * (n - 1) * out["d_singles"]["paths"]
        out["accept_a_lt_d"] = dict(a=a, d=d, holds=bool(a < d))
        out["cond_a_le_d_minus_generators"] = dict(a=a, bound=bound, holds=bool(a <= bound))
        out["block_order"] = dict(banded=a, plain=b, banded_over_plain=a / b)
        out["one_per_launch_over_default"] = c / a
        assert out["a_chain"]["delta0"] == out["b_other_order"]["delta0"] == out["c_one_per_launch"]["delta0"] == \
            out["d_singles"]["delta0"]
    print(json.dumps(out), flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(json.dumps(out) + "\n")


def main(argv):
    out_file, root = None, ROOT
    for flag in ("--out", "--root"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--out":
                out_file = os.path.abspath(argv[i + 1])
            else:
                root = os.path.abspath(argv[i + 1])
            argv = argv[:i] + argv[i + 2:]
    baseline = "--baseline" in argv
    if argv and argv[0] == "--one":
        M, N, n = (int(v) for v in argv[1:4])
        return one(M, N, n, argv[4], int(argv[5]), int(argv[6]), baseline, root, out_file)
    nums = [int(v) for v in argv if not v.startswith("--")]
    reps, warm = (nums + [5, 2][len(nums):])[:2]
    for M, N, n, kind in CONFIGS:
        if baseline and kind == "schedules":
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(M), str(N), str(n), kind, str(reps), str(warm),
               "--root", root]
        if baseline:
            cmd.append("--baseline")
        if out_file:
            cmd += ["--out", out_file]
        try:
            rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"time_chain_greeks: {M} x {N} x {n} {kind} ran out of time ({LIMIT_S} s); nothing more is started", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"time_chain_greeks: {M} x {N} x {n} {kind} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

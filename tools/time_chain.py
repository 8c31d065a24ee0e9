"""Cost of a whole American option chain (omc_price_american_chain) against the ways to price the same quotes without it.

Headline: 1M paths x 252 steps, GBM, S0 = 100, 8 puts at K = 80 .. 115 in steps of 5; then 16 entries (K = 80 .. 117.5 in
steps of 2.5), and both again at 131,072 x 50.  Per configuration, in ONE process, alternating, medians of `reps` after
`warm` warm-ups of the HIP-event time of the whole call (first launch to last completion):
    (a) the chain, fused sweeps            (b) the chain, unfused (the single-strike sweeps per entry on the shared matrix)
    (c) omc_price_american_seq of the same pricings (x n: its ms_total is per pricing)      (d) n single calls, summed
and ms_paths of (c), the generator of one pricing.  The two conditions of the chain's design are evaluated and printed:
    (b) <= (c) - 0.8 (n - 1) ms_paths(c)   -- the unfused chain banks at least the generators it no longer runs
    (a) <= (b)                             -- the fused sweeps beat the single-strike ones
One JSON line per configuration, on stdout and appended to --out FILE; the committed record is profiles/chain_time.txt
(this build's lines, then the --baseline lines of a build of the parent commit).  Every configuration runs in a child process of its own under a time limit, and the
first one that fails or runs out of time ends the run (nothing more is started on the GPU after a fault).
usage: time_chain.py [--baseline] [--out FILE] [reps] [warm]
--baseline: (c) and (d) only -- what a build without the chain entry points can run (their code is shared).
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/time_chain.py --one M N n reps warm`."""
import json
import os
import statistics as st
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1_000_000, 252, 8), (1_000_000, 252, 16), (131_072, 50, 8), (131_072, 50, 16)]
LIMIT_S = 240


def strikes(n):
    return [80.0 + 40.0 / n * i for i in range(n)]  # 8: steps of 5; 16: steps of 2.5


def one(M, N, n, reps, warm, baseline, out_file=None):
    sys.path.insert(0, ROOT)
    from options_model_amd import _ffi
    ctx = _ffi.default_context(0)
    ks = strikes(n)
    ps = [_ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, K=K, seed=42) for K in ks]

    def chain(fused):
        ctx.set_option("chain_fused", fused)
        outs, info = ctx.price_american_chain(ps[0], ks, True)
        return dict(total=info["ms_total"], paths=info["ms_paths"], pass1=info["ms_pass1"], pass2=info["ms_pass2"],
                    fused=info["fused"], launches=info["n_launch_groups"], price0=outs[0]["price"])

    def seq():
        outs = ctx.price_american_seq(ps)
        return dict(total=outs[0]["ms_total"] * n, paths=outs[0]["ms_paths"], price0=outs[0]["price"])

    def singles():
        outs = [ctx.price_american(p) for p in ps]
        return dict(total=sum(o["ms_total"] for o in outs), paths=st.median(o["ms_paths"] for o in outs),
                    price0=outs[0]["price"])

    runs = {"c_seq": seq, "d_singles": singles}
    if not baseline:
        runs = {"a_fused": lambda: chain(1), "b_unfused": lambda: chain(0), **runs}
    samples = {k: [] for k in runs}
    for it in range(warm + reps):
        for k, fn in runs.items():  # alternating: every variant sees the same state of the machine
            r = fn()
            if it >= warm:
                samples[k].append(r)
    out = dict(build="baseline" if baseline else "chain", M=M, N=N, n=n, reps=reps, warm=warm)
    for k, rs in samples.items():
        out[k] = {f: st.median(r[f] for r in rs) for f in rs[0]}
        out[k]["min_total"] = min(r["total"] for r in rs)
    if not baseline:
        a, b, c = out["a_fused"]["total"], out["b_unfused"]["total"], out["c_seq"]["total"]
        bound = c - 0.8 * (n - 1) * out["c_seq"]["paths"]
        out["width"] = ctx.chain_width(ps[0], n)
        out["cond_b_le_c_minus_generators"] = dict(b=b, bound=bound, holds=bool(b <= bound))
        out["cond_a_le_b"] = dict(a=a, b=b, holds=bool(a <= b))
        assert out["a_fused"]["price0"] == out["b_unfused"]["price0"] == out["c_seq"]["price0"] == out["d_singles"]["price0"]
    print(json.dumps(out), flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(json.dumps(out) + "\n")


def main(argv):
    out_file = None
    if "--out" in argv:
        i = argv.index("--out")
        out_file = os.path.abspath(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    if argv and argv[0] == "--one":
        M, N, n, reps, warm = (int(v) for v in argv[1:6])
        return one(M, N, n, reps, warm, "--baseline" in argv, out_file)
    baseline = "--baseline" in argv
    nums = [int(v) for v in argv if not v.startswith("--")]
    reps, warm = (nums + [5, 2])[:2] if len(nums) < 2 else nums[:2]
    for M, N, n in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(M), str(N), str(n), str(reps), str(warm)]
        if baseline:
            cmd.append("--baseline")
        if out_file:
            cmd += ["--out", out_file]
        try:
            rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"time_chain: {M} x {N} x {n} ran out of time ({LIMIT_S} s); nothing more is started", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"time_chain: {M} x {N} x {n} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

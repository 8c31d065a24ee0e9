#!/usr/bin/env python3
"""A fixed, seeded list of small pricings that reaches every host launcher of the backward-induction sweeps.

Run it under a kernel trace (rocprofv3 --kernel-trace -- python tools/launch_trace.py) on two builds: the ordered list of
(kernel name, grid, workgroup, LDS bytes) shows which kernel and geometry every dispatch picked, and the lines printed
here -- every result's sums as float64 hex, and its counters -- show what they computed.  A change of the launch layer
alone leaves both the same, line for line.  `--compare A.csv B.csv` does the first comparison on two kernel-trace files.

Default environment only; apart from the one shape that selects the 16-byte folded pass 2, N <= 12 and M <= 20002.
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOWS = ("reference", "textbook", "two_pass")
FLOAT_KEYS = ("price", "sum", "sumsq")
COUNT_KEYS = ("n_paths", "n_exercised", "n_zero", "sum_nitm", "folded")


def show(label, d, extra=()):
    parts = [f"{k}={float(d[k]).hex()}" for k in FLOAT_KEYS + tuple(extra)] + [f"{k}={int(d[k])}" for k in COUNT_KEYS if k in d]
    print(f"{label}: " + " ".join(parts), flush=True)


def run():
    sys.path.insert(0, ROOT)
    import numpy as np
    from options_model_amd import _ffi

    ctx = _ffi.Context(0)
    mk = _ffi.make_params
    K, R, SIG, T = 100.0, 0.05, 0.2, 1.0

    # -- backward induction on a given matrix: 16-byte rows, M % 4 != 0, and a leading dimension that alone forces scalar
    for M, ld in ((4096, 4096), (1002, 1002), (1004, 1007)):
        N = 9
        rng = np.random.default_rng(5)
        z = rng.standard_normal((N, M))
        dt = T / N
        S = np.zeros((N + 1, ld), np.float32)
        S[0, :M] = 100.0
        S[1:, :M] = 100.0 * np.exp(np.cumsum((R - 0.5 * SIG * SIG) * dt + SIG * np.sqrt(dt) * z, axis=0))
        Sd = ctx.to_device(S)
        for sem in FLOWS:
            for put in (True, False):
                show(f"lsm_poly M={M} ld={ld} {sem} {'put' if put else 'call'}",
                     ctx.lsm_poly(Sd, K, R, T, put, sem, n_paths=M))
        Sd.free()

    # -- fused pricing on the antithetic-folded matrix: 16-byte, scalar (odd column count), and the 16-byte pass 2
    ctx.set_option("fold_antithetic", 2)
    for M, N in ((8192, 12), (20002, 12), (4194312, 4)):
        for put in (True, False):
            show(f"fused folded M={M} N={N} {'put' if put else 'call'}",
                 ctx.price_american(mk(semantics="two_pass", is_put=put, n_paths=M, n_steps=N, seed=7, stream=1)))
    # chain (the default route: the single sweeps per entry) and Greeks on the folded matrix
    chain = mk(semantics="two_pass", n_paths=8192, n_steps=10, seed=9)
    strikes, sides = [90.0, 95.0, 100.0, 105.0, 110.0], [True, False, True, True, False]
    out, info = ctx.price_american_chain(chain, strikes, sides)
    print("chain folded info: " + " ".join(f"{k}={v}" for k, v in sorted(info.items()) if not k.startswith("ms")), flush=True)
    for k, o in zip(strikes, out):
        show(f"chain folded K={k}", o)
    for M in (8192, 20002):
        show(f"greeks folded M={M}", ctx.price_american_greeks(mk(semantics="two_pass", n_paths=M, n_steps=10, seed=3)),
             extra=("delta", "gamma", "vega", "rho", "theta"))
    # a two-pass sequence on folded matrices (its small launches grouped)
    seq = [mk(semantics="two_pass", is_put=bool(i % 2), n_paths=8192, n_steps=10, K=95.0 + 3 * i, seed=20 + i) for i in range(4)]
    print(f"seq two_pass folded group width: {ctx.seq_group_width(seq)}", flush=True)
    for i, o in enumerate(ctx.price_american_seq(seq)):
        show(f"seq two_pass folded [{i}]", o)
    ctx.set_option("fold_antithetic", 0)
    out, info = ctx.price_american_chain(chain, strikes, sides)
    for k, o in zip(strikes, out):
        show(f"chain full K={k}", o)
    for M in (8192, 1002):
        show(f"greeks full M={M}", ctx.price_american_greeks(mk(semantics="two_pass", is_put=False, n_paths=M, n_steps=10, seed=3)),
             extra=("delta", "gamma", "vega", "rho", "theta"))
    ctx.set_option("fold_antithetic", 1)

    # -- a per-step sweep replayed from its captured graph
    ctx.set_option("step_graph", 1)
    for sem, M in (("reference", 4096), ("reference", 4096), ("textbook", 4096), ("textbook", 1002)):
        show(f"step graph {sem} M={M}", ctx.price_american(mk(semantics=sem, n_paths=M, n_steps=8, seed=31)))
    ctx.set_option("step_graph", -1)

    # -- sequences of 4 pricings of one geometry: per-step (shared launches per time step) and two-pass
    for sem in ("reference", "textbook", "two_pass"):
        for M in (4096, 1002):
            seq = [mk(semantics=sem, is_put=bool(i % 2), n_paths=M, n_steps=10, K=95.0 + 3 * i, seed=40 + i) for i in range(4)]
            print(f"seq {sem} M={M} widths: step={ctx.seq_step_width(seq)} group={ctx.seq_group_width(seq)}", flush=True)
            for i, o in enumerate(ctx.price_american_seq(seq)):
                show(f"seq {sem} M={M} [{i}]", o)

    # -- batches: 6 members of mixed sizes in each flow, ContNet, European
    sizes = ((4096, 9), (1002, 7), (6, 1), (2000, 12), (10000, 5), (20002, 3))
    for sem in FLOWS:
        ps = [mk(semantics=sem, is_put=bool(i % 2), n_paths=M, n_steps=N, S0=95.0 + 2 * i, T=0.5, seed=50 + i, stream=i)
              for i, (M, N) in enumerate(sizes)]
        for i, o in enumerate(ctx.price_american_batch(ps)):
            show(f"batch {sem} [{i}]", o)
    ps = [mk(semantics="reference", is_put=bool(i % 2), n_paths=M, n_steps=N, S0=98.0 + 2 * i, T=0.5, seed=60 + i, stream=i)
          for i, (M, N) in enumerate(((2000, 4), (1002, 3), (4096, 4)))]
    for i, o in enumerate(ctx.price_american_contnet_batch(ps, 32, 2, 1e-3, 7)):
        show(f"contnet batch [{i}]", o)
    for model, scheme in (("gbm", "reference"), ("heston", "reference"), ("heston", "full_truncation"), ("heston", "calibrator")):
        ps = [mk(model=model, heston_scheme=scheme, is_put=bool(i % 2), n_paths=M, n_steps=N, seed=70 + i, stream=i)
              for i, (M, N) in enumerate(((4096, 9), (1002, 7), (20002, 12)))]
        for i, o in enumerate(ctx.price_european_batch(ps)):
            show(f"european batch {model} {scheme} [{i}]", o)
    ctx.close()


def dispatches(path):
    """the ordered (kernel, grid, workgroup, LDS bytes) of a rocprofv3 kernel-trace csv"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r["Dispatch_Id"])))
    lds = "Dynamic_LDS_Block_Size" if rows and "Dynamic_LDS_Block_Size" in rows[0] else "LDS_Block_Size"
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"),
             int(r[lds])) for r in rows]


def compare(a_path, b_path):
    a, b = dispatches(a_path), dispatches(b_path)
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    print(f"dispatches: {len(a)} and {len(b)}; differing lines: {len(diff) + abs(len(a) - len(b))}")
    print(f"distinct kernels dispatched: {len({x[0] for x in a})} and {len({x[0] for x in b})}")
    for i, x, y in diff[:20]:
        print(f"  line {i}: {x} != {y}")
    return 0 if not diff and len(a) == len(b) else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()

"""HIP-event cost of one omc_price_barrier call against one omc_price_american on full storage (option
"fold_antithetic" = 0, the storage the barrier pricing always uses) at 1M x 252, GBM put, the calls alternated in one
process.  Cases: discrete down-and-out American (H = 90), the same with continuous monitoring, and the European-only
discrete down-and-out (no matrix).  Prints one JSON line per case: median event times of the whole call and of its
kernels, and the ratio to the vanilla pricing.  usage: time_barrier.py [reps] [M N]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/time_barrier.py`."""
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
M, N = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (1_000_000, 252)
ctx = _ffi.default_context(0)
ctx.set_option("fold_antithetic", 0)
p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=42)
cases = {
    "down_out_discrete_american": dict(kind="down-and-out", H=90.0, monitoring="discrete", american=True),
    "down_out_continuous_american": dict(kind="down-and-out", H=90.0, monitoring="continuous", american=True),
    "down_out_discrete_european": dict(kind="down-and-out", H=90.0, monitoring="discrete", american=False),
}
for name, kw in cases.items():
    ctx.price_american(p)
    ctx.price_barrier(p, **kw)  # warm-up: code objects, workspaces
    a, b = [], []
    for _ in range(reps):
        a.append(ctx.price_american(p))
        b.append(ctx.price_barrier(p, **kw))
    med = lambda rs, k: st.median(r[k] for r in rs)  # noqa: E731
    out = dict(case=name, M=M, N=N, reps=reps,
               vanilla_full_ms=dict(total=med(a, "ms_total"), paths=med(a, "ms_paths"), pass1=med(a, "ms_pass1"),
                                    pass2=med(a, "ms_pass2")),
               barrier_ms=dict(total=med(b, "ms_total"), barrier_paths=med(b, "ms_barrier_paths"),
                               pass1=med(b, "ms_pass1"), pass2=med(b, "ms_pass2")),
               ratio_total=med(b, "ms_total") / med(a, "ms_total"),
               ratio_paths=med(b, "ms_barrier_paths") / med(a, "ms_paths"),
               price=b[0]["price"], n_exercised=b[0]["n_exercised"], euro_out=b[0]["euro_out"],
               hit_prob=b[0]["hit_prob"])
    print(json.dumps(out), flush=True)

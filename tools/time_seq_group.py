"""Two-pass sequences in groups: HIP-event time per pricing against the group width (option seq_two_pass_k) and the
pricing's size.  Per size the widths take turns, one 64-pricing sequence each, until every cell has a second of work:
the box drifts by more than the effect over a job, so the columns of a row are taken side by side.
usage: time_seq_group.py [n_steps] [paths,paths,...] [k,k,...]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from options_model_amd import _ffi

N = int(sys.argv[1]) if len(sys.argv) > 1 else 252
SIZES = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [65_536, 262_144, 1_000_000, 8_000_000]
KS = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [1, 2, 4, 8, 16]
SEQ = 64

ctx = _ffi.Context(0)
print(f"ms per pricing (first launch to last completion / {SEQ}), GBM put, two-pass, folded, {N} steps; median [min] over the "
      f"sequences of a cell; K = option seq_two_pass_k (width the library reports)", flush=True)
for M in SIZES:
    ps = [_ffi.make_params(semantics="two_pass", n_paths=M, n_steps=N, seed=42, stream=i) for i in range(SEQ)]
    width, ms = {}, {k: [] for k in KS}
    for k in KS:                                   # buffers and code objects warm
        ctx.set_option("seq_two_pass_k", k)
        width[k] = ctx.seq_group_width(ps)
        ctx.price_american_seq(ps[:max(2, min(width[k], SEQ))])
    while min(sum(v) for v in ms.values()) * SEQ < 1000.0:
        for k in KS:
            ctx.set_option("seq_two_pass_k", k)
            ms[k].append(ctx.price_american_seq(ps)[0]["ms_total"])
    ctx.set_option("seq_two_pass_k", -1)
    base = statistics.median(ms[KS[0]])
    cells = "  ".join(f"K {k:2d} ({width[k]:2d}): {statistics.median(ms[k]):.4f} [{min(ms[k]):.4f}] "
                      f"{base / statistics.median(ms[k]):.3f}x" for k in KS)
    print(f"paths {M:9d} ({len(ms[KS[0]])} sequences per cell, default width {ctx.seq_group_width(ps)}): {cells}", flush=True)
ctx.close()

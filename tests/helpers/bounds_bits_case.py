"""The cases of tests/test_gpu_bounds_bits.py and of tools/capture_bounds_bits.py, which recorded them at the commit before
the bound kernels' shared bodies (omc_bounds_dev.h): one call per bound kernel, small enough for a few seconds in all.
TEST INFRASTRUCTURE ONLY.

Every case: N = 5 (one full Philox block and a partial one), n_outer = 16, n_lower = 1024, n_inner = 160 (80 pairs on 64
lanes: the refill runs), the policy textbook (fitted on 2048 paths) or given.  The vanilla entry for put and call; the
basket entry for d = 1 .. 8 with the kind rotating and basket_bounds_case.unequal_basket's law.  One case of each entry
sets pass2_tables_irregular_every = 2, so bd_stop's float64 rule is taken too.
"""
from __future__ import annotations

import hashlib

import numpy as np

from helpers import basket_bounds_case as bc
from options_model_amd import _ffi

N, N_OUTER, N_LOWER, N_INNER, M = 5, 16, 1024, 160, 2048
K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
FLOATS = ("lower", "se_lower", "upper", "se_upper")
COUNTS = ("n_exercised_lower", "inner_path_steps")
ARRAYS = ("q", "samples")


def cases():
    out = [dict(name="vanilla-put", d=0, kind=None, is_put=True, policy="given", irr_every=2),
           dict(name="vanilla-call", d=0, kind=None, is_put=False, policy="textbook", irr_every=0)]
    for d in range(1, 9):
        kind = bc.KINDS[(d - 1) % 3]
        out.append(dict(name=f"basket-d{d}-{kind}", d=d, kind=kind, is_put=d % 2 == 1,
                        policy=("textbook", "given")[(d - 1) // 2 % 2], irr_every=2 if d == 3 else 0))
    return out


def _vanilla_given(ctx, p):
    """a policy from other paths (stream 9), textbook fits"""
    S = ctx.gbm_paths(M, N, 100.0, R, SIG, T, 42, 9)
    d = ctx.lsm_poly(S, K, R, T, bool(p.is_put), "textbook")
    S.free()
    t = np.zeros((N + 1, 4))
    t[:, :3], t[:, 3] = d["betas"], d["nitm"]
    return t


def run(ctx, case):
    """-> the recorded fields of one case: float.hex() of the bounds and errors, the counts, SHA-256 of q and samples"""
    p = _ffi.make_params(model="gbm", is_put=case["is_put"], semantics="two_pass", n_paths=M, n_steps=N, S0=100.0, K=K, r=R,
                         sigma=SIG, T=T, seed=42, stream=0)
    kw = dict(policy=case["policy"], n_lower=N_LOWER, n_outer=N_OUTER, n_inner=N_INNER, want_q=True, want_samples=True)
    ctx.set_option("pass2_tables_irregular_every", case["irr_every"])
    try:
        if case["d"] == 0:
            if case["policy"] == "given":
                kw["betas"] = _vanilla_given(ctx, p)
            r = ctx.price_american_bounds(p, **kw)
        else:
            b = bc.unequal_basket(case["d"], case["kind"])
            if case["policy"] == "given":
                kw["betas"] = bc.fuzz_given_table(ctx, p, b, np.zeros(N + 1, bool))
            r = ctx.price_american_basket_bounds(p, b, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    out = {k: float(r[k]).hex() for k in FLOATS}
    out.update({k: int(r[k]) for k in COUNTS})
    out.update({k + "_sha256": hashlib.sha256(np.ascontiguousarray(r[k], np.float64).tobytes()).hexdigest() for k in ARRAYS})
    return out

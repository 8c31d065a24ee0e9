"""The cases of the dividend Greeks' tests and what the CPU and GPU tests share to run them: the
schedules of the issue's list as (step, amount, kind) entries, the device calls that produce the three scenario matrices and
the normals, and the comparison of a result with the restatement (helpers/dividend_greeks_ref.py).  TEST INFRASTRUCTURE
ONLY.
"""
import math

import numpy as np

from helpers import dividend_bounds_case as dc
from helpers import dividend_greeks_ref as gr
from helpers import dividend_ref as dr

C, P = "cash", "proportional"
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
HP_QE = dict(v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)  # Feller violated: both branches of the QE step
MODELS = ("gbm", "heston0", "heston1", "heston3")
RAGGED = 2 * (3 * 256 + 5)  # a ragged last workgroup of the one-lane-per-pair sweep

# name -> steps(N): the schedules of the list.  Step 4 | 5 is a Philox-block boundary under GBM, 2 | 3 under Heston.
SCHEDULES = {
    "cash": lambda N: [(2, 1.5, C), (4, 1.0, C)],
    "proportional": lambda N: [(3, 0.03, P), (5, 0.02, P)],
    "mixed": lambda N: [(2, 1.0, C), (3, 0.02, P), (4, 2.0, C), (5, 1.0, C)],
    "two-on-one-step": lambda N: [(3, 1.0, C), (3, 0.02, P), (3, 0.5, C)],
    "step-1-and-N": lambda N: [(1, 2.0, C), (N, 1.5, C), (N, 0.01, P)],
    "floor": lambda N: [(3, 92.0, C)],
}
FLOOR_ALL = [(2, 1000.0, C)]  # takes every path to 0


def hp_of(model):
    return HP_QE if model == "heston3" else HP


def make_params(model, **kw):
    kw.setdefault("hp", hp_of(model))
    return dc.make_params(model, **kw)


def device_inputs(ctx, p, q, divs, h):
    """-> ((S, S_up, S_down) host float32 matrices of omc_price_american_div's S_keep at S0, S0 (1 + h), S0 (1 - h), their
    result dicts, Z: the generator's normals [N][M/2] under GBM, else None)"""
    N, M = int(p.n_steps), int(p.n_paths)
    mats, res = [], []
    for lam in (1.0, 1.0 + h, 1.0 - h):
        S = ctx.empty((N + 1, M), np.float32)
        try:
            res.append(ctx.price_american_div(dc.with_(p, S0=p.S0 * lam), q, divs, S_keep=S))
            mats.append(S.to_host())
        finally:
            S.free()
    Z = None
    if not dc.is_heston(p):
        Zd = ctx.gbm_normals(M // 2, N, p.seed, p.stream, p.pair_offset)
        Z = Zd.to_host()
        Zd.free()
    return mats, res, Z


def restate(p, q, divs, h, mats, Z, betas4):
    mul, cash, has = dr.schedule(p.T, int(p.n_steps), divs)
    return gr.greeks(mats, p.K, p.r, q, p.T, bool(p.is_put), betas4, mul, cash, has, h,
                     sigma=p.sigma if Z is not None else None, Z=Z)


def rel_errors(out, ref, gbm, names=None):
    """{greek: |device - restatement| / |restatement|} (0 where both are exactly 0)"""
    err = {}
    for g in names or (gr.GREEKS if gbm else ("delta", "gamma")):
        a, b = out[g], ref[g]
        err[g] = 0.0 if a == b else abs(a - b) / abs(b) if b != 0.0 else math.inf
    return err


def stop_at(N, step):
    """a policy that stops every in-the-money path at `step` (0: nowhere -- the European option)"""
    b = np.zeros((N + 1, 4))
    if 1 <= step < N:
        b[step] = (-1e30, 0.0, 0.0, 1.0)
    return b


def fuzz_cases(n, seed=20261021):
    """n seeded cases: random schedules of 0 .. 5 dividends (cash and proportional, random steps, repeats allowed), N in
    2 .. 13, a ragged even n_paths, models cycled, put / call, a yield on every other case"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        N = int(rng.integers(2, 14))
        divs = []
        for _ in range(int(rng.integers(0, 6))):
            k = int(rng.integers(1, N + 1))
            divs.append((k, float(rng.uniform(0.0, 4.0)), C) if rng.integers(0, 2) else (k, float(rng.uniform(0.0, 0.06)), P))
        out.append(dict(model=MODELS[c % len(MODELS)], N=N, M=2 * int(rng.integers(200, 1200)), is_put=bool(rng.integers(0, 2)),
                        q=0.03 if c % 2 else 0.0, divs=divs, seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 8)),
                        S0=float(rng.uniform(92.0, 108.0)), h=float(rng.choice([0.005, 0.01, 0.05]))))
    return out

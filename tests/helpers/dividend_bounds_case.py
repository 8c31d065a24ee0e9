"""What the dividend bound tests share (omc_price_american_bounds_div, omc_dividend_paths_f32).
TEST INFRASTRUCTURE ONLY.

The device's own spots for the numpy restatements of tests/helpers/bounds_ref.py, bounds_schedule_ref.py and
bounds_check_ref.py, from Context.dividend_paths at the documented Philox coordinates:
  lower paths   n_lower paths at stream_lower, pair_offset 0
  outer paths   n_outer paths at stream_outer, pair_offset 0, under Heston with the variance state: So, Vo
  inner paths   of item (i, t): rows 0 .. N-t of the n_inner paths of N steps started at (So[t, i], Vo[t, i]) at date t
                (step_offset = t) at stream_inner, pair_offset g = (i (N+1) + t) n_inner / 2 (a float32 is exact in the double
                argument; v0 is a start state there, so a negative scheme-1 state passes)
Device and libm exp2 / sqrt differ by an ulp, so the comparison is on the device's own spots, as the other bound tests do it.
And the directed cases of tests/test_gpu_dividend_bounds.py with the seeded case generator of
tests/test_gpu_dividend_bounds_fuzz.py, which need no GPU (tests/test_dividend_bounds_cpu.py).

A case names its dividends by STEP: (step, amount, kind).  dividends_of puts each in the middle of its step's interval,
t = (step - 0.5) T / N, which omc_dividend_schedule maps back to that step.
"""
from __future__ import annotations

import numpy as np

from helpers import bounds_schedule_ref as bsr
from helpers import heston_bounds_case as hc
from helpers import jump_bounds_case as jc

MODELS = jc.MODELS
POLICIES = hc.POLICIES
HP, HP_CLAMP = hc.HP, hc.HP_CLAMP
N_INNER = (2, 64, 130, 200)
host = hc.host
make_params, with_, is_heston = jc.make_params, jc.with_, jc.is_heston
check_against_restatement = hc.check_against_restatement


def dividends_at(steps, T, N):
    """[(step, amount, kind)] -> [(t, amount, kind)] with t in the middle of the step's interval"""
    return [((k - 0.5) * T / N, float(a), kind) for k, a, kind in steps]


def dividends_of(case):
    return dividends_at(case["divs"], case["T"], case["N"])


def steps_of(case):
    """the ex-dividend steps of a case, sorted, one entry per step"""
    return sorted({k for k, _, _ in case["divs"]})


def case_params(case):
    return make_params(case["model"], is_put=case["is_put"], S0=case["S0"], K=case["K"], r=case["r"], sigma=case["sigma"],
                       T=case["T"], N=case["N"], M=case["M"], seed=case["seed"], stream=case["stream"], hp=case["hp"])


def fitted_table(ctx, p, q, divs, policy, k=0):
    """omc_lsm_poly's fits with semantics `policy` on the device's own dividend paths of p -> betas4 [N+1][4]; k >= 2: on the
    gathered rows with the schedule's horizon, scattered to the scheduled rows (bounds_schedule_ref.fitted_table's rule)"""
    N = int(p.n_steps)
    S = host(ctx.dividend_paths(p, q, divs))
    G = ctx.to_device(bsr.gather(S, k))
    d = ctx.lsm_poly(G, p.K, p.r, bsr.horizon(p.T, N, k), bool(p.is_put), policy)
    G.free()
    t = np.zeros((N + 1, 4))
    rows = bsr.schedule(N, k)
    t[rows, :3], t[rows, 3] = d["betas"], d["nitm"]
    if int(k) >= 2:
        t[0] = 0.0
    return t


def given_table(ctx, p, q, divs, holes=None):
    """a policy from other paths (2048 of stream 9 of p's seed), textbook fits, with n = 0 on the dates `holes` marks"""
    t = fitted_table(ctx, with_(p, n_paths=2048, stream=9, pair_offset=0), q, divs, "textbook")
    if holes is not None:
        t[np.asarray(holes), 3] = 0.0
    return t


def inner_item(ctx, p, q, divs, So, Vo, n_inner, stream_inner, i, t):
    """the inner spots of item (i, t): [N - t + 1][n_inner]"""
    N = int(p.n_steps)
    g = (i * (N + 1) + t) * (n_inner // 2)
    kw = dict(n_paths=n_inner, S0=float(So[t, i]), stream=stream_inner, pair_offset=g)
    if Vo is not None:
        kw["v0"] = float(Vo[t, i])
    return host(ctx.dividend_paths(with_(p, **kw), q, divs, step_offset=t))[:N - t + 1]


def device_spots(ctx, p, q, divs, n_lower, n_outer, n_inner, ts=None, streams=None):
    """-> dict Sl (lower paths), So, Vo (outer spots / variance state; Vo None under GBM) and inner(i, t) -> [N - t + 1][n_inner]
    spots, every item of the dates `ts` (None: 0 .. N-1) computed once"""
    N = int(p.n_steps)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Sl = host(ctx.dividend_paths(with_(p, n_paths=n_lower, stream=s_lo, pair_offset=0), q, divs))
    po = with_(p, n_paths=n_outer, stream=s_out, pair_offset=0)
    if is_heston(p):
        Sd, Vd = ctx.dividend_paths(po, q, divs, want_v=True)
        So, Vo = host(Sd), host(Vd)
    else:
        So, Vo = host(ctx.dividend_paths(po, q, divs)), None
    ts = range(N) if ts is None else ts
    items = {(i, t): inner_item(ctx, p, q, divs, So, Vo, n_inner, s_in, i, t) for i in range(n_outer) for t in ts}
    return dict(Sl=Sl, So=So, Vo=Vo, inner=lambda i, t: items[(i, t)])


# ---------------------------------------------------------------------------------------------- the directed cases
def _case(model, N, n_inner, n_outer, is_put, policy, q, divs, irr_every=0, seed=42, hp=HP, S0=100.0):
    c = dict(model=model, N=N, n_inner=n_inner, n_outer=n_outer, n_lower=1000, M=2000, is_put=is_put, policy=policy, q=q,
             divs=divs, irr_every=irr_every, seed=seed, stream=0, hp=hp, S0=S0, K=100.0, r=0.05, sigma=0.2, T=1.0)
    c["holes"] = [t % 3 == 1 for t in range(N + 1)]  # dates of a given table with n = 0
    return c


C, P = "cash", "proportional"
# N in {1, 2, 4, 5, 9, 13}; n_inner in {2, 64, 130, 200}; n_outer in {2, 6, 40}; put and call; the four policies; cash,
# proportional and mixed schedules; q in {0, 0.03}; the three models; the float64 fallback (irr_every); the absorbing zero.
# What the schedules contain between them is asserted in tests/test_dividend_bounds_cpu.py.
DIRECTED = [
    _case("gbm", 9, 64, 6, True, "textbook", 0.03, [(4, 2.0, C), (5, 1.5, C), (9, 0.02, P)]),
    _case("gbm", 13, 130, 6, False, "two_pass", 0.0, [(1, 3.0, C), (1, 0.03, P), (8, 2.0, C)], S0=104.0),
    _case("gbm", 5, 200, 2, True, "reference", 0.0, [(3, 0.05, P)], irr_every=2),
    _case("gbm", 1, 2, 40, True, "given", 0.03, [(1, 1.0, C)]),
    _case("gbm", 4, 64, 40, False, "textbook", 0.03, [(2, 2.0, C), (2, 0.01, P), (3, 1.0, C)], S0=104.0),
    _case("heston0", 9, 64, 6, True, "textbook", 0.0, [(2, 2.0, C), (3, 2.0, C), (9, 0.02, P)]),
    _case("heston0", 4, 130, 6, False, "given", 0.03, [(1, 4.0, C), (4, 1.0, C)], S0=104.0),
    _case("heston0", 2, 2, 40, True, "two_pass", 0.0, [(1, 0.1, P)]),
    _case("heston1", 13, 200, 2, True, "reference", 0.03, [(1, 1.0, C), (6, 1.0, C), (7, 1.0, C), (13, 1.0, C)], hp=HP_CLAMP),
    _case("heston1", 5, 64, 6, False, "textbook", 0.0, [(2, 3.0, C), (3, 0.02, P)], irr_every=3, S0=104.0, hp=HP_CLAMP),
    _case("heston1", 9, 130, 2, True, "given", 0.03, [(5, 2.0, C), (5, 0.03, P)]),
    _case("gbm", 9, 64, 6, True, "textbook", 0.0, [(3, 95.0, C), (6, 1.0, C)]),       # the absorbing zero
    _case("heston0", 5, 130, 6, False, "textbook", 0.0, [(2, 97.0, C), (4, 0.5, P)]),  # the same under Heston, a call
]
ABSORBING = DIRECTED[-2:]


def case_id(c):
    d = "+".join(f"{k}{kind[0]}" for k, _, kind in c["divs"])
    return f"{c['model']}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{'put' if c['is_put'] else 'call'}-{c['policy']}-{d}"


# ---------------------------------------------------------------------------------------------- the fuzz cases
def fuzz_cases(n, seed=20261021):
    """n seeded cases of the fuzz sweep, as plain dicts: random schedules of 0 .. 5 dividends (cash and proportional, on
    random steps, repeats allowed), N in 1 .. 13, n_inner of N_INNER, a ragged even n_outer up to 40, models and policies
    cycled, put / call, the float64 fallback on some, every third case with a schedule (`every`), every third with the payoff
    check (`check`)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        N = int(rng.integers(1, 14))
        kappa, theta = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.01, 0.09))
        bound = float(np.sqrt(2.0 * kappa * theta))  # Feller: xi below it
        xi = bound * float(rng.uniform(1.3, 3.0)) if c % 4 == 2 else bound * float(rng.uniform(0.2, 0.9))
        hp = dict(v0=float(rng.uniform(0.01, 0.09)), kappa=kappa, theta=theta, xi=xi, rho=float(rng.uniform(-0.9, 0.5)))
        divs = []
        for _ in range(int(rng.integers(0, 6))):
            if rng.integers(0, 2):
                divs.append((int(rng.integers(1, N + 1)), float(rng.uniform(0.2, 4.0)), C))
            else:
                divs.append((int(rng.integers(1, N + 1)), float(rng.uniform(0.002, 0.05)), P))
        case = dict(model=MODELS[(c + c // 3) % 3], N=N, n_inner=N_INNER[3 - c % 4], n_outer=2 * int(rng.integers(1, 21)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy=POLICIES[(c + c // 4) % 4], divs=divs,
                    q=float(rng.choice((0.0, 0.0, 0.02, 0.05))), irr_every=int(rng.choice((0, 0, 1, 2, 3))),
                    seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)), hp=hp,
                    S0=100.0 * float(rng.uniform(0.8, 1.25)), K=100.0, r=float(rng.uniform(0.0, 0.08)),
                    sigma=float(rng.uniform(0.1, 0.4)), T=float(rng.uniform(0.5, 3.0)))
        case["holes"] = [bool(v) for v in rng.random(N + 1) < 0.3]
        case["every"] = int(rng.integers(2, N + 4)) if c % 3 == 1 else 0
        case["check"] = "payoff" if c % 3 == 2 else None
        case["refill"] = case["n_inner"] // 2 > 64
        out.append(case)
    return out

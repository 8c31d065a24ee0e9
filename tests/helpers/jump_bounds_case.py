"""What the jump-diffusion bound tests share (omc_price_american_bounds_jump, omc_jump_paths_f32).
TEST INFRASTRUCTURE ONLY.

The device's own spots for the numpy restatements of tests/helpers/bounds_ref.py, bounds_schedule_ref.py and
bounds_check_ref.py, from Context.jump_paths at the documented Philox coordinates:
  lower paths   n_lower paths at stream_lower, pair_offset 0
  outer paths   n_outer paths at stream_outer, pair_offset 0, under Heston with the variance state: So, Vo
  inner paths   of item (i, t): rows 0 .. N-t of the n_inner paths of N steps started at (So[t, i], Vo[t, i]) at
                stream_inner, pair_offset g = (i (N+1) + t) n_inner / 2 (a float32 is exact in the double argument; v0 is a
                start state there, so a negative scheme-1 state passes)
Device and libm exp2 / sqrt differ by an ulp, so the comparison is on the device's own spots, as the other bound tests do it.
And the directed cases of tests/test_gpu_jump_bounds.py with the seeded case generator of tests/test_gpu_jump_bounds_fuzz.py,
which need no GPU (tests/test_jump_bounds_cpu.py).
"""
from __future__ import annotations

import numpy as np

from helpers import bounds_schedule_ref as bsr
from helpers import heston_bounds_case as hc
from options_model_amd import _ffi

MODELS = ("gbm", "heston0", "heston1")
POLICIES = hc.POLICIES
HP, HP_CLAMP = hc.HP, hc.HP_CLAMP
N_INNER = (2, 64, 130, 200)
host = hc.host


def make_params(model, is_put=True, S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, N=8, M=2000, seed=42, stream=0, hp=HP):
    if model == "gbm":
        return _ffi.make_params(model="gbm", is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N, S0=S0, K=K, r=r,
                                sigma=sigma, T=T, seed=seed, stream=stream)
    return _ffi.make_params(model="heston", heston_scheme=int(model[-1]), is_put=is_put, semantics="two_pass", n_paths=M,
                            n_steps=N, S0=S0, K=K, r=r, sigma=0.0, T=T, seed=seed, stream=stream, **hp)


def with_(p, **kw):
    """a copy of p with the fields of kw set"""
    q = type(p).from_buffer_copy(bytes(p))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def is_heston(p):
    return p.model != _ffi.MODELS["gbm"]


def jump_of(case):
    """(lambda, mu_j, sigma_j) of a case: lambda from x = lambda T / N"""
    return (case["x"] * case["N"] / case["T"], case["mu_j"], case["sigma_j"])


def case_params(case):
    return make_params(case["model"], is_put=case["is_put"], S0=case["S0"], K=case["K"], r=case["r"], sigma=case["sigma"],
                       T=case["T"], N=case["N"], M=case["M"], seed=case["seed"], stream=case["stream"], hp=case["hp"])


def fitted_table(ctx, p, jump, q, policy, k=0):
    """omc_lsm_poly's fits with semantics `policy` on the device's own jump paths of p -> betas4 [N+1][4]; k >= 2: on the
    gathered rows with the schedule's horizon, scattered to the scheduled rows (bounds_schedule_ref.fitted_table's rule)"""
    N = int(p.n_steps)
    S = host(ctx.jump_paths(p, jump, q))
    G = ctx.to_device(bsr.gather(S, k))
    d = ctx.lsm_poly(G, p.K, p.r, bsr.horizon(p.T, N, k), bool(p.is_put), policy)
    G.free()
    t = np.zeros((N + 1, 4))
    rows = bsr.schedule(N, k)
    t[rows, :3], t[rows, 3] = d["betas"], d["nitm"]
    if int(k) >= 2:
        t[0] = 0.0
    return t


def given_table(ctx, p, jump, q, holes=None):
    """a policy from other paths (2048 of stream 9 of p's seed), textbook fits, with n = 0 on the dates `holes` marks"""
    t = fitted_table(ctx, with_(p, n_paths=2048, stream=9, pair_offset=0), jump, q, "textbook")
    if holes is not None:
        t[np.asarray(holes), 3] = 0.0
    return t


def inner_item(ctx, p, jump, q, So, Vo, n_inner, stream_inner, i, t):
    """the inner spots of item (i, t): [N - t + 1][n_inner]"""
    N = int(p.n_steps)
    g = (i * (N + 1) + t) * (n_inner // 2)
    kw = dict(n_paths=n_inner, S0=float(So[t, i]), stream=stream_inner, pair_offset=g)
    if Vo is not None:
        kw["v0"] = float(Vo[t, i])
    return host(ctx.jump_paths(with_(p, **kw), jump, q))[:N - t + 1]


def device_spots(ctx, p, jump, q, n_lower, n_outer, n_inner, ts=None, streams=None):
    """-> dict Sl (lower paths), So, Vo (outer spots / variance state; Vo None under GBM) and inner(i, t) -> [N - t + 1][n_inner]
    spots, every item of the dates `ts` (None: 0 .. N-1) computed once"""
    N = int(p.n_steps)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Sl = host(ctx.jump_paths(with_(p, n_paths=n_lower, stream=s_lo, pair_offset=0), jump, q))
    po = with_(p, n_paths=n_outer, stream=s_out, pair_offset=0)
    if is_heston(p):
        Sd, Vd = ctx.jump_paths(po, jump, q, want_v=True)
        So, Vo = host(Sd), host(Vd)
    else:
        So, Vo = host(ctx.jump_paths(po, jump, q)), None
    ts = range(N) if ts is None else ts
    items = {(i, t): inner_item(ctx, p, jump, q, So, Vo, n_inner, s_in, i, t) for i in range(n_outer) for t in ts}
    return dict(Sl=Sl, So=So, Vo=Vo, inner=lambda i, t: items[(i, t)])


check_against_restatement = hc.check_against_restatement


# ---------------------------------------------------------------------------------------------- the directed cases
def _case(model, N, n_inner, n_outer, is_put, policy, x, q, irr_every=0, seed=42, hp=HP, mu_j=-0.1, sigma_j=0.15, S0=100.0):
    c = dict(model=model, N=N, n_inner=n_inner, n_outer=n_outer, n_lower=1000, M=2000, is_put=is_put, policy=policy, x=x,
             q=q, irr_every=irr_every, seed=seed, stream=0, hp=hp, mu_j=mu_j, sigma_j=sigma_j, S0=S0, K=100.0, r=0.05,
             sigma=0.2, T=1.0)
    c["holes"] = [t % 3 == 1 for t in range(N + 1)]  # dates of a given table with n = 0
    return c


# N in {1, 2, 4, 5, 9, 13}; n_inner in {2, 64, 130, 200}; n_outer in {2, 6, 40}; put and call; the four policies; lambda T / N
# in {0.01, 0.3, 1.0}; q in {0, 0.03}; the three models; the float64 fallback (irr_every)
DIRECTED = [
    _case("gbm", 9, 64, 6, True, "textbook", 0.3, 0.03),
    _case("gbm", 13, 130, 6, False, "two_pass", 1.0, 0.0, S0=104.0),
    _case("gbm", 5, 200, 2, True, "reference", 0.01, 0.0, irr_every=2),
    _case("gbm", 1, 2, 40, True, "given", 0.3, 0.03),
    _case("gbm", 4, 64, 40, False, "textbook", 1.0, 0.03, S0=104.0),
    _case("heston0", 9, 64, 6, True, "textbook", 0.3, 0.0),
    _case("heston0", 4, 130, 6, False, "given", 1.0, 0.03, S0=104.0),
    _case("heston0", 2, 2, 40, True, "two_pass", 0.01, 0.0),
    _case("heston1", 13, 200, 2, True, "reference", 1.0, 0.03, hp=HP_CLAMP),  # (xi = 1: negative variance states)
    _case("heston1", 5, 64, 6, False, "textbook", 0.3, 0.0, irr_every=3, S0=104.0, hp=HP_CLAMP),
    _case("heston1", 9, 130, 2, True, "given", 0.01, 0.03),
    _case("heston1", 1, 64, 6, True, "textbook", 1.0, 0.0, hp=HP_CLAMP),
]


def case_id(c):
    return f"{c['model']}-N{c['N']}-i{c['n_inner']}-o{c['n_outer']}-{'put' if c['is_put'] else 'call'}-{c['policy']}-x{c['x']}"


def wave_counts(philox, case, i=0, t=0):
    """jump counts of the first item wave of item (i, t) of a case -> int64 [N+1][min(64, n_inner / 2)] from
    jump_ref.draws at the inner pairs' coordinates (row k: inner step k; rows after N - t are not simulated)"""
    from helpers import jump_ref as jr

    N, H = case["N"], case["n_inner"] // 2
    lam, mu, sj = jump_of(case)
    thr = jr.table(lam, mu, sj, case["r"], case["q"], case["T"], N)[0]
    n, _ = jr.draws(philox, min(64, H), N, case["seed"], case["stream"] + 3, (i * (N + 1) + t) * H, thr)
    return n


# ---------------------------------------------------------------------------------------------- the fuzz cases
def fuzz_cases(n, seed=20261020):
    """n seeded cases of the fuzz sweep, as plain dicts: random laws and lambda T / N in (0, 1], N in 1 .. 13, n_inner of
    N_INNER, a ragged even n_outer up to 40, models and policies cycled, put / call, the float64 fallback on some, every
    third case with a schedule (`every`), every third with the payoff check (`check`)."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        N = int(rng.integers(1, 14))
        kappa, theta = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.01, 0.09))
        bound = float(np.sqrt(2.0 * kappa * theta))  # Feller: xi below it
        xi = bound * float(rng.uniform(1.3, 3.0)) if c % 4 == 2 else bound * float(rng.uniform(0.2, 0.9))
        hp = dict(v0=float(rng.uniform(0.01, 0.09)), kappa=kappa, theta=theta, xi=xi, rho=float(rng.uniform(-0.9, 0.5)))
        case = dict(model=MODELS[(c + c // 3) % 3], N=N, n_inner=N_INNER[3 - c % 4], n_outer=2 * int(rng.integers(1, 21)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy=POLICIES[(c + c // 4) % 4],
                    x=float(1.0 - rng.uniform(0.0, 1.0) ** 2), q=float(rng.choice((0.0, 0.0, 0.02, 0.05))),
                    irr_every=int(rng.choice((0, 0, 1, 2, 3))), seed=int(rng.integers(1, 1 << 31)),
                    stream=int(rng.integers(0, 50)), hp=hp, mu_j=float(rng.uniform(-0.3, 0.1)),
                    sigma_j=float(rng.uniform(0.0, 0.3)), S0=100.0 * float(rng.uniform(0.8, 1.25)), K=100.0,
                    r=float(rng.uniform(0.0, 0.08)), sigma=float(rng.uniform(0.1, 0.4)), T=float(rng.uniform(0.5, 3.0)))
        case["x"] = max(case["x"], 1e-3)
        case["holes"] = [bool(v) for v in rng.random(N + 1) < 0.3]
        case["every"] = int(rng.integers(2, N + 4)) if c % 3 == 1 else 0
        case["check"] = "payoff" if c % 3 == 2 else None
        case["refill"] = case["n_inner"] // 2 > 64
        out.append(case)
    return out

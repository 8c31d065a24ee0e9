"""What the barrier bound tests share (omc_price_american_bounds_barrier, omc_barrier_paths_state_f32; DESIGN.md section
31).  TEST INFRASTRUCTURE ONLY.

The device's own REAL spots for the restatement of tests/helpers/barrier_bounds_ref.py, built as
heston_bounds_case.device_spots builds them -- the vanilla generators at the documented Philox coordinates, gbm_normals and
the *_paths_from_normals entry points started at the outer state -- so the barrier generator under test takes no part in its
own reference; barrier_bounds_ref encodes them with the start's hit state.
  lower paths   n_lower vanilla paths at stream_lower, pair_offset 0
  outer paths   n_outer vanilla paths at stream_outer, pair_offset 0, under Heston with the variance state: So, Vo
  inner paths   of item (i, t): the normals of stream_inner at pair offset (i (N+1) + t) n_inner / 2 through the from-normals
                entry point started at (So[t, i], Vo[t, i]), rows 0 .. N-t
And the SHAPES and directed CASES of tests/test_gpu_barrier_bounds.py with the seeded case generator of
tests/test_gpu_barrier_bounds_fuzz.py, which need no GPU: tests/test_barrier_bounds_cpu.py asserts on the C oracle's paths
(the same Philox coordinates, float32 spots within an ulp or two of the device's) that every shape and barrier meets the
conditions the cases are there for.
"""
from __future__ import annotations

import numpy as np

from helpers import barrier_bounds_ref as bbr
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bsr
from helpers import heston_bounds_case as hc
from helpers import jump_bounds_case as jc
from options_model_amd import _ffi

MODELS = jc.MODELS
POLICIES = hc.POLICIES
HP, HP_CLAMP = hc.HP, hc.HP_CLAMP
N_INNER = (2, 64, 130, 200)
KINDS = bbr.KINDS
MODES = ("plain", "scheduled", "payoff")
host = hc.host
make_params, with_, is_heston = jc.make_params, jc.with_, jc.is_heston


# ---------------------------------------------------------------------------------------------- the shapes
# One shape per model carries the full product kinds x put / call x modes; the spots of a shape depend on neither, so a
# module computes them once.  N in {1, 2, 3, 7, 13}, n_inner in {2, 64, 130, 200} (130 and 200: more pairs than a wave has
# lanes, the refill), n_outer even, ragged and at most 40.  H_down / H_up are placed so that the conditions of
# tests/test_barrier_bounds_cpu.py hold for the shape's own seeds; `every` is the schedule of the scheduled mode.
# (n_inner = 2 goes with N = 3, not with N = 1: with one date the upper bound is the plain mean of n_outer n_inner <= 80
# payoffs, of which a barrier near the money leaves a handful non-zero -- too few for a standard error that the ordering check
# upper >= lower - 3 (se_lower + se_upper) can lean on; with more dates the estimator's upward bias takes over.)
def _shape(name, model, N, n_inner, n_outer, H_down, H_up, every, seed, n_lower=600, M=2000, hp=HP, sigma=0.2, T=1.0):
    return dict(name=name, model=model, N=N, n_inner=n_inner, n_outer=n_outer, n_lower=n_lower, M=M, H_down=H_down, H_up=H_up,
                every=every, seed=seed, stream=0, hp=hp, S0=100.0, K=100.0, r=0.05, sigma=sigma, T=T)


SHAPES = {s["name"]: s for s in [
    _shape("gbm-7", "gbm", 7, 64, 38, 93.0, 107.0, 3, 42),
    _shape("h0-3", "heston0", 3, 2, 26, 93.0, 108.0, 2, 43),
    _shape("h1-7", "heston1", 7, 130, 22, 97.0, 103.0, 2, 64, hp=HP_CLAMP),
    _shape("gbm-13", "gbm", 13, 130, 40, 95.0, 106.0, 5, 55),
    _shape("h0-1", "heston0", 1, 200, 40, 97.0, 112.0, 2, 46),  # (one step: partners multiply to ~ 103^2)
    _shape("h1-2", "heston1", 2, 64, 34, 95.0, 106.0, 2, 47, hp=HP_CLAMP),
]}
FULL = ("gbm-7", "h0-3", "h1-7")  # the full product
SIDE = ("gbm-13", "h1-2", "h0-1")  # the remaining N and n_inner, four cases each


def barrier_of(shape, kind):
    return shape["H_down"] if kind.startswith("down") else shape["H_up"]


def _case(shape, kind, is_put, mode, policy):
    return dict(shape=shape, kind=kind, is_put=is_put, mode=mode, policy=policy)


CASES = [_case(s, kind, is_put, mode, POLICIES[(a + b + c) % 4])
         for s in FULL for a, kind in enumerate(KINDS) for b, is_put in enumerate((True, False)) for c, mode in enumerate(MODES)]
# (N = 1 has no item that starts hit, so "h0-1" carries the knock-outs alone; with one date a schedule is the plain game)
CASES += [_case("gbm-13", KINDS[j], j % 2 == 0, MODES[j % 3], POLICIES[(j + 1) % 4]) for j in range(4)]
CASES += [_case("h1-2", KINDS[3 - j], j % 2 == 1, MODES[(j + 1) % 3], POLICIES[(j + 2) % 4]) for j in range(4)]
CASES += [_case("h0-1", KINDS[j % 2], j < 2, MODES[2 * (j % 2)], POLICIES[j]) for j in range(4)]


def case_id(c):
    return f"{c['shape']}-{c['kind']}-{'put' if c['is_put'] else 'call'}-{c['mode']}-{c['policy']}"


def shape_params(shape, is_put=True):
    return make_params(shape["model"], is_put=is_put, S0=shape["S0"], K=shape["K"], r=shape["r"], sigma=shape["sigma"],
                       T=shape["T"], N=shape["N"], M=shape["M"], seed=shape["seed"], stream=shape["stream"], hp=shape["hp"])


def mode_args(shape, mode):
    """-> (exercise_every, suboptimality_check) of a mode"""
    return (shape["every"], None) if mode == "scheduled" else (0, "payoff" if mode == "payoff" else None)


# ---------------------------------------------------------------------------------------------- the device's own spots
def vanilla_paths(ctx, p, want_v=False):
    """the vanilla generator's paths of p on the host -> S, or (S, V) under Heston with want_v"""
    n, N = int(p.n_paths), int(p.n_steps)
    if not is_heston(p):
        return host(ctx.gbm_paths(n, N, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, p.pair_offset))
    if want_v:
        S, V = ctx.heston_paths_sv(n, N, p.S0, p.r, p.T, *hc.hp_of(p), p.seed, p.stream, p.pair_offset, int(p.heston_scheme))
        return host(S), host(V)
    return host(ctx.heston_paths(n, N, p.S0, p.r, p.T, *hc.hp_of(p), p.seed, p.stream, p.pair_offset, int(p.heston_scheme)))


def device_spots(ctx, p, n_lower, n_outer, n_inner, ts=None, streams=None):
    """-> dict Sl (REAL lower paths), So, Vo (REAL outer spots / variance state; Vo None under GBM) and inner(i, t) -> the REAL
    inner spots [N - t + 1][n_inner], every item of the dates `ts` (None: 0 .. N-1) computed once.  The spots depend on the law,
    the seed and the streams of p, not on the contract, the payoff or the policy."""
    N = int(p.n_steps)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Sl = vanilla_paths(ctx, with_(p, n_paths=n_lower, stream=s_lo, pair_offset=0))
    po = with_(p, n_paths=n_outer, stream=s_out, pair_offset=0)
    if is_heston(p):
        So, Vo = vanilla_paths(ctx, po, want_v=True)
        kappa, theta, xi, rho = hc.hp_of(p)[1:]
        inner = hc.inner_from_state(lambda off, n: host(ctx.gbm_normals(n, 2 * N, p.seed, s_in, off)),
                                    lambda z1, z2, s0, v0: host(ctx.heston_paths_from_normals(z1, z2, s0, p.r, p.T, v0, kappa,
                                                                                                theta, xi, rho,
                                                                                                int(p.heston_scheme))),
                                    So, Vo, n_inner)
    else:
        So, Vo = vanilla_paths(ctx, po), None
        inner = br.inner_by_item(lambda off, n: host(ctx.gbm_normals(n, N, p.seed, s_in, off)), So, n_inner,
                                 lambda z, s0: host(ctx.gbm_paths_from_normals(z, s0, p.r, p.sigma, p.T)))
    ts = range(N) if ts is None else ts
    items = {(i, t): inner(i, t) for i in range(n_outer) for t in ts}
    return dict(Sl=Sl, So=So, Vo=Vo, inner=lambda i, t: items[(i, t)])


def barrier_fit_matrix(ctx, p, kind, H):
    """omc_price_barrier's kept ENCODED matrix of p's fitting paths, on the host"""
    S = ctx.empty((int(p.n_steps) + 1, int(p.n_paths)), np.float32)
    ctx.price_barrier(p, kind, H, american=True, keep_paths=S)
    return host(S)


def fitted_table(ctx, p, kind, H, policy, k=0):
    """omc_lsm_poly's fits with semantics `policy` on omc_price_barrier's encoded matrix of p -> betas4 [N+1][4]; k >= 2: on
    the gathered rows with the schedule's horizon, scattered to the scheduled rows (bounds_schedule_ref.fitted_table's rule)"""
    N = int(p.n_steps)
    G = ctx.to_device(bsr.gather(barrier_fit_matrix(ctx, p, kind, H), k))
    d = ctx.lsm_poly(G, p.K, p.r, bsr.horizon(p.T, N, k), bool(p.is_put), policy)
    G.free()
    t = np.zeros((N + 1, 4))
    rows = bsr.schedule(N, k)
    t[rows, :3], t[rows, 3] = d["betas"], d["nitm"]
    if int(k) >= 2:
        t[0] = 0.0
    return t


def given_table(ctx, p, holes=None, scale_call=0.9):
    """a table [N+1][4] that does stop paths early: textbook fits on 2048 VANILLA paths of stream 9 (a policy need not know
    the barrier), n = 0 on the dates `holes` marks; for a call with the continuation values scaled down"""
    t = bsr.given_table(ctx, p, holes)
    if not p.is_put:
        t[:, :3] *= scale_call
    return t


def holes_of(N):
    return [t % 3 == 1 for t in range(N + 1)]


# ---------------------------------------------------------------------------------------------- the oracle's view of a shape
def oracle_outer(shape):
    """the C oracle's outer paths of a shape (stream + 2, pair offset 0): REAL float32 spots [N+1][n_outer]"""
    from oracle import cpu as orc
    s = shape
    if s["model"] == "gbm":
        return orc.gbm_paths(s["n_outer"], s["N"], s["S0"], s["r"], s["sigma"], s["T"], s["seed"], s["stream"] + 2)
    hp = s["hp"]
    return orc.heston_paths(s["n_outer"], s["N"], s["S0"], s["r"], s["T"], hp["v0"], hp["kappa"], hp["theta"], hp["xi"],
                            hp["rho"], s["seed"], s["stream"] + 2, 0, int(s["model"][-1]))


def oracle_item0(shape, i=0):
    """the C oracle's inner paths of item (i, 0) -- the start is (S0, v0) whatever i -- [N+1][n_inner]"""
    from oracle import cpu as orc
    s = shape
    g = i * (s["N"] + 1) * (s["n_inner"] // 2)
    if s["model"] == "gbm":
        return orc.gbm_paths(s["n_inner"], s["N"], s["S0"], s["r"], s["sigma"], s["T"], s["seed"], s["stream"] + 3, g)
    hp = s["hp"]
    return orc.heston_paths(s["n_inner"], s["N"], s["S0"], s["r"], s["T"], hp["v0"], hp["kappa"], hp["theta"], hp["xi"],
                            hp["rho"], s["seed"], s["stream"] + 3, g, int(s["model"][-1]))


# ---------------------------------------------------------------------------------------------- the fuzz cases
def fuzz_cases(n, seed=20261023):
    """n seeded cases of the fuzz sweep, as plain dicts: the four kinds cycled, N in 1 .. 13, n_inner of N_INNER, a ragged even
    n_outer up to 40, models and policies cycled, put / call, the float64 fallback on some, every third case with a schedule
    (`every`), every third with the payoff check (`check`); the barrier a random 2 .. 10 % away from the spot"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        N = int(rng.integers(1, 14))
        kappa, theta = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.01, 0.09))
        bound = float(np.sqrt(2.0 * kappa * theta))  # Feller: xi below it
        xi = bound * float(rng.uniform(1.3, 3.0)) if c % 4 == 2 else bound * float(rng.uniform(0.2, 0.9))
        hp = dict(v0=float(rng.uniform(0.01, 0.09)), kappa=kappa, theta=theta, xi=xi, rho=float(rng.uniform(-0.9, 0.5)))
        kind = KINDS[(c + c // 4) % 4]
        S0 = 100.0 * float(rng.uniform(0.9, 1.1))
        gap = float(rng.uniform(0.02, 0.10))
        case = dict(model=MODELS[(c + c // 3) % 3], kind=kind, H=S0 * (1.0 - gap if kind.startswith("down") else 1.0 + gap), N=N,
                    n_inner=N_INNER[3 - c % 4], n_outer=2 * int(rng.integers(1, 21)), n_lower=2 * int(rng.integers(100, 700)),
                    M=2 * int(rng.integers(300, 1500)), is_put=bool(rng.integers(0, 2)), policy=POLICIES[(c + c // 4) % 4],
                    irr_every=int(rng.choice((0, 0, 1, 2, 3))), seed=int(rng.integers(1, 1 << 31)),
                    stream=int(rng.integers(0, 50)), hp=hp, S0=S0, K=100.0, r=float(rng.uniform(0.0, 0.08)),
                    sigma=float(rng.uniform(0.1, 0.4)), T=float(rng.uniform(0.5, 3.0)))
        case["holes"] = [bool(v) for v in rng.random(N + 1) < 0.3]
        case["every"] = int(rng.integers(2, N + 4)) if c % 3 == 1 else 0
        case["check"] = "payoff" if c % 3 == 2 else None
        case["refill"] = case["n_inner"] // 2 > 64
        out.append(case)
    return out


def case_params(case):
    return make_params(case["model"], is_put=case["is_put"], S0=case["S0"], K=case["K"], r=case["r"], sigma=case["sigma"],
                       T=case["T"], N=case["N"], M=case["M"], seed=case["seed"], stream=case["stream"], hp=case["hp"])


def unreachable(kind):
    """a barrier no float32 path of these tests reaches"""
    return 1e-3 if kind.startswith("down") else 1e9

"""The cases of the jump Greeks' tests and what the CPU and GPU tests share to run them: the
grid of the issue's list, the device calls that produce the three scenario matrices and the normals, the counts and
jump normals from the C oracle's Philox, and the comparison of a result with the restatement
(helpers/jump_greeks_ref.py).  TEST INFRASTRUCTURE ONLY.
"""
import itertools
import math

import numpy as np

from helpers import jump_bounds_case as jc
from helpers import jump_greeks_ref as gr
from helpers import jump_ref as jr

HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
HP_QE = dict(v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)  # Feller violated: both branches of the QE step
MODELS = ("gbm", "heston0", "heston1", "heston3")
PAIRS = (1, 63, 64, 65, 257, 773)    # one lane; a wave less one, exactly, plus one; a workgroup plus one; a ragged fourth
STEPS = (1, 2, 3, 4, 5, 8, 9, 13)    # a count block ends on the step / one before it; Heston's half block falls odd
XS = (1e-6, 0.05, 1.0)               # x = lambda T / N: no wave takes the branch, mixed waves, every lane jumps
SIZES = ((-0.1, 0.15), (0.2, 0.0), (0.0, 0.3), (0.0, 0.0))
T, Q = 1.0, 0.02
with_, is_heston = jc.with_, jc.is_heston


def hp_of(model):
    return HP_QE if model == "heston3" else HP


def make_params(model, **kw):
    kw.setdefault("hp", hp_of(model))
    return jc.make_params(model, **kw)


def grid():
    """every (model, steps) once; pairs, x, sizes and put / call cycled at strides that cover every (x, sizes), (model, x)
    and (pairs, x) combination (checked in tests/test_jump_greeks_cpu.py)"""
    out = []
    for i, (m, s) in enumerate(itertools.product(range(len(MODELS)), range(len(STEPS)))):
        law = (3 * i + i // 12) % 12  # (x, sizes) as one index
        out.append(dict(model=MODELS[m], N=STEPS[s], pairs=PAIRS[(i + i // 6) % 6], x=XS[law // 4], sizes=SIZES[law % 4],
                        is_put=(i + i // 2) % 2 == 0, seed=300 + i, stream=i % 5))
    return out


def case_id(c):
    return (f"{c['model']}-N{c['N']}-P{c['pairs']}-x{c['x']}-mu{c['sizes'][0]}-sj{c['sizes'][1]}-"
            f"{'put' if c['is_put'] else 'call'}")


def jump_of(c):
    """(lambda, mu_j, sigma_j): lambda from x = lambda T / N"""
    return (c["x"] * c["N"] / c.get("T", T), c["sizes"][0], c["sizes"][1])


def case_params(c):
    return make_params(c["model"], is_put=c["is_put"], N=c["N"], M=2 * c["pairs"], seed=c["seed"], stream=c["stream"],
                       sigma=c.get("sigma", 0.25), S0=c.get("S0", 100.0), T=c.get("T", T), r=c.get("r", 0.05))


def device_inputs(ctx, p, jump, q, h):
    """-> ((S, S_up, S_down) host float32 matrices of omc_price_american_jump's S_keep at S0, S0 (1 + h), S0 (1 - h), their
    result dicts, Z: the generator's normals [N][M/2] under GBM, else None).  lambda > 0: full storage."""
    N, M = int(p.n_steps), int(p.n_paths)
    mats, res = [], []
    for lam in (1.0, 1.0 + h, 1.0 - h):
        S = ctx.empty((N + 1, M), np.float32)
        try:
            res.append(ctx.price_american_jump(with_(p, S0=p.S0 * lam), jump, q, S_keep=S))
            mats.append(S.to_host())
        finally:
            S.free()
    Z = None
    if not is_heston(p):
        Zd = ctx.gbm_normals(M // 2, N, p.seed, p.stream, p.pair_offset)
        Z = Zd.to_host()
        Zd.free()
    return mats, res, Z


def oracle_draws(p, jump, q):
    """counts and jump normals [N+1][M/2] of p's pairs from the C oracle's Philox"""
    from oracle import cpu as orc

    lam, mu, sj = jump
    thr = jr.table(lam, mu, sj, p.r, q, p.T, int(p.n_steps))[0]
    return gr.draws(orc.philox_words, int(p.n_paths) // 2, int(p.n_steps), int(p.seed), int(p.stream), int(p.pair_offset), thr)


def restate(p, jump, q, h, mats, Z, betas4):
    lam, mu, sj = jump
    n = zJ = None
    if Z is not None:
        n, zJ = oracle_draws(p, jump, q)
    return gr.greeks(mats, p.S0, p.K, p.r, q, p.T, bool(p.is_put), betas4, h, lam, mu, sj,
                     sigma=p.sigma if Z is not None else None, Z=Z, n=n, zJ=zJ)


def rel_errors(out, ref, names):
    """{greek: |device - restatement| / |restatement|} (0 where both are exactly 0)"""
    err = {}
    for g in names:
        a, b = out[g], ref[g]
        err[g] = 0.0 if a == b else abs(a - b) / abs(b) if b != 0.0 else math.inf
    return err


def european(N):
    """the policy that exercises nowhere: the European option"""
    return np.zeros((N + 1, 4))


def fuzz_cases(n, seed=20261022):
    """n seeded cases: ragged pair counts up to 1200, N in 1 .. 13, random laws and x in (0, 1], models cycled, put / call,
    a yield on every other case, three bump sizes"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        N = int(rng.integers(1, 14))
        out.append(dict(model=MODELS[c % len(MODELS)], N=N, pairs=int(rng.integers(100, 1201)), is_put=bool(rng.integers(0, 2)),
                        q=0.03 if c % 2 else 0.0, x=max(1e-3, float(1.0 - rng.uniform(0.0, 1.0) ** 2)),
                        sizes=(float(rng.uniform(-0.3, 0.1)), float(rng.uniform(0.0, 0.3))),
                        seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 8)),
                        S0=float(rng.uniform(92.0, 108.0)), h=float(rng.choice([0.005, 0.01, 0.05])),
                        sigma=float(rng.uniform(0.1, 0.4)), T=float(rng.uniform(0.5, 3.0)), r=float(rng.uniform(0.0, 0.08))))
    return out


# ---------------------------------------------------------------------------------------------- the European case
EURO = dict(S0=100.0, K=100.0, r=0.05, q=0.02, sigma=0.2, T=1.0, N=8, M=1 << 18, lam=2.0, mu_j=-0.1, sigma_j=0.15, seed=42,
            stream=0, h=0.01)
EURO_NAMES = ("price", "delta", "vega", "rho", "dmu_j", "dsigma_j", "dlambda", "theta")


def euro_params(is_put):
    e = EURO
    return make_params("gbm", is_put=is_put, S0=e["S0"], K=e["K"], r=e["r"], sigma=e["sigma"], T=e["T"], N=e["N"], M=e["M"],
                       seed=e["seed"], stream=e["stream"])


def euro_closed_form(is_put):
    """Merton's series and its central differences in float64, valued at t = dt as the two-pass flow values a path that is
    never exercised early (D[N-1], as the dividend Greeks' European test does): exp(r T / N) merton(..).  The series is
    analytic: a central difference of 1e-6 relative (absolute for mu_j) is good to 1e-9."""
    e = EURO
    x0 = dict(S0=e["S0"], r=e["r"], sigma=e["sigma"], T=e["T"], lam=e["lam"], mu_j=e["mu_j"], sigma_j=e["sigma_j"])

    def f(**kw):
        a = dict(x0, **kw)
        return math.exp(a["r"] * a["T"] / e["N"]) * jr.merton(a["S0"], e["K"], a["r"], e["q"], a["sigma"], a["T"], a["lam"],
                                                               a["mu_j"], a["sigma_j"], is_put)

    def d(name):
        eps = 1e-6 * max(abs(x0[name]), 0.1)
        return (f(**{name: x0[name] + eps}) - f(**{name: x0[name] - eps})) / (2.0 * eps)

    return dict(price=f(), delta=d("S0"), vega=d("sigma"), rho=d("r"), dmu_j=d("mu_j"), dsigma_j=d("sigma_j"),
                dlambda=d("lam"), theta=-d("T"))


def euro_restatement(is_put):
    """the float64 restatement of the European case on float64 paths from the C oracle's Philox: its normals, counts and
    jump normals"""
    from oracle import cpu as orc

    e = EURO
    P, N = e["M"] // 2, e["N"]
    Z = orc.gbm_normals(P, N, e["seed"], e["stream"], 0).astype(np.float64)
    thr = jr.table(e["lam"], e["mu_j"], e["sigma_j"], e["r"], e["q"], e["T"], N)[0]
    n, zJ = gr.draws(orc.philox_words, P, N, e["seed"], e["stream"], 0, thr)
    law = (e["lam"], e["mu_j"], e["sigma_j"])
    S3 = [gr.simulate(e["S0"] * f, e["r"], e["q"], e["sigma"], e["T"], N, Z, n, zJ, *law) for f in (1.0, 1.0 + e["h"], 1.0 - e["h"])]
    return gr.greeks(S3, e["S0"], e["K"], e["r"], e["q"], e["T"], is_put, european(N), e["h"], *law, sigma=e["sigma"], Z=Z,
                     n=n, zJ=zJ)

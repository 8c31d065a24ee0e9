"""numpy restatement of the price bounds of a game with an exercise SCHEDULE (option "bounds_exercise_every" = k; the
definitions are in DESIGN.md section 25 and include/omc.h), built on tests/helpers/bounds_ref.py.  TEST INFRASTRUCTURE ONLY.

The scheduled dates of a grid of N steps are tau_j = N - (J - j) k, j = 1 .. J = (N - 1) // k + 1, and tau_0 = 0.  A policy
table whose rows off the schedule are zero (n = 0) never stops a path there, so bounds_ref.first_stop on the masked table IS
the scheduled stopping time, on the paths of the fine grid; what this file adds is the schedule itself, the inner items at
the scheduled dates only, the walk over the scheduled dates, the gathered matrix of the fit, the device's own spots for the
scheduled items and the seeded cases of tests/test_gpu_bounds_schedule_fuzz.py.
"""
from __future__ import annotations

import math

import numpy as np

from helpers import bounds_ref as br
from helpers import heston_bounds_case as hc
from options_model_amd import _ffi


# ---------------------------------------------------------------------------------------------- the schedule
def schedule(N, k):
    """-> [tau_0 = 0, tau_1, .., tau_J]; k = 0 or 1 is every date"""
    N, k = int(N), int(k)
    if k < 0:
        raise ValueError("exercise_every must be a non-negative integer.")
    if k < 2:
        return list(range(N + 1))
    return [0] + [t for t in range(1, N + 1) if (N - t) % k == 0]


def n_dates(N, k):
    return len(schedule(N, k)) - 1


def horizon(T, N, k):
    """T_v of the fit on the gathered matrix: T when J k == N, else T (J k) / N"""
    if int(k) < 2:
        return T
    Jk = n_dates(N, k) * int(k)
    return T if Jk == int(N) else T * float(Jk) / float(int(N))


def mask(betas4, k):
    """the table with zero rows off the schedule (row 0 is no exercise date); k < 2: a copy"""
    b = np.array(betas4, np.float64)
    if int(k) < 2:
        return b
    N = b.shape[0] - 1
    out = np.zeros_like(b)
    on = schedule(N, k)[1:]
    out[on] = b[on]
    return out


def gather(S, k):
    """rows 0, tau_1 .. tau_J of a path matrix [N+1][m]: what the policy is fitted on"""
    return np.ascontiguousarray(S[schedule(S.shape[0] - 1, k)])


def max_inner_steps(N, k, n_outer, n_inner):
    """the inner steps of a policy that never exercises: n_outer n_inner sum_{j<J} (N - tau_j)"""
    return int(n_outer) * int(n_inner) * sum(int(N) - t for t in schedule(N, k)[:-1])


# ---------------------------------------------------------------------------------------------- the estimators
def q_rows(So, inner, rows, K, r, T, is_put, betas4, k):
    """Q^ of the outer paths in `rows` at the dates tau_0 .. tau_{J-1} -> dict q [len(rows)][N] (zero off those columns),
    inner_path_steps, ties.  inner(i, t) as bounds_ref.upper_bound takes it, asked for at scheduled t only."""
    N = So.shape[0] - 1
    bk = mask(betas4, k)
    q = np.zeros((len(rows), N))
    steps = ties = 0
    for m, i in enumerate(rows):
        for t in schedule(N, k)[:-1]:
            tau, Z, ti = br.first_stop(inner(i, t), t, N, K, r, T, is_put, bk)
            q[m, t] = Z.sum() / Z.size
            steps += int((tau - t).sum())
            ties += ti
    return dict(q=q, inner_path_steps=steps, ties=ties)


def walk_rows(So, q, rows, K, r, T, is_put, betas4, k):
    """The walk over the scheduled dates with q [len(rows)][N] (columns tau_j read): M_0 = 0, M_j = M_{j-1} + L_j - Q_{j-1},
    L_j = Z_{tau_j} where the policy exercises or j = J, else Q_j -> dict samples, ties, zmax, M [len(rows)][J+1]."""
    N = So.shape[0] - 1
    bk = mask(betas4, k)
    taus = schedule(N, k)
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    samples = np.zeros(len(rows))
    Ms = np.zeros((len(rows), len(taus)))
    ties = 0
    zmax = 0.0
    for m, i in enumerate(rows):
        M, best = 0.0, -math.inf
        for j in range(1, len(taus)):
            t = taus[j]
            s = So[t, i:i + 1]
            phi = (K - float(s[0])) if is_put else (float(s[0]) - K)
            Zt = D[t] * max(phi, 0.0)
            zmax = max(zmax, Zt)
            st, ti = br.stop_rule(s, t, N, K, is_put, bk)
            ties += ti
            qt = q[m, t] if t < N else 0.0
            L = Zt if st[0] else qt
            M = M + L - q[m, taus[j - 1]]
            Ms[m, j] = M
            best = max(best, Zt - M)
        samples[m] = best
    return dict(samples=samples, ties=ties, zmax=zmax, M=Ms)


def upper_bound(So, inner, K, r, T, is_put, betas4, k):
    rows = range(So.shape[1])
    qr = q_rows(So, inner, rows, K, r, T, is_put, betas4, k)
    wk = walk_rows(So, qr["q"], rows, K, r, T, is_put, betas4, k)
    up, se, ratio = br._pair_mean_se(wk["samples"])
    return dict(upper=up, se_upper=se, se_cancel=ratio, q=qr["q"], samples=wk["samples"],
                inner_path_steps=qr["inner_path_steps"], ties=qr["ties"] + wk["ties"], zmax=wk["zmax"])


def lower_bound(S, K, r, T, is_put, betas4, k):
    return br.lower_bound(S, K, r, T, is_put, mask(betas4, k))


def check_against_restatement(p, dev, sp, k, n_lower, n_outer, n_inner, rtol=1e-12):
    """heston_bounds_case.check_against_restatement for the scheduled game: the device's dict `dev` (want_q, want_samples)
    against the restatement on the device's own spots `sp` (Sl, So, inner): no ties, equal counts, q / samples / bounds at rtol
    (atol rtol K, as tests/test_gpu_bounds.py)."""
    K, is_put = float(p.K), bool(p.is_put)
    lo = lower_bound(sp["Sl"], K, p.r, p.T, is_put, dev["betas"], k)
    up = upper_bound(sp["So"], sp["inner"], K, p.r, p.T, is_put, dev["betas"], k)
    assert lo["ties"] == 0 and up["ties"] == 0  # numpy's decisions are the device's
    assert dev["n_exercised_lower"] == lo["n_exercised"]
    assert dev["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(dev["q"], up["q"], rtol=rtol, atol=rtol * K)
    np.testing.assert_allclose(dev["samples"], up["samples"], rtol=rtol, atol=rtol * K)
    for key in ("lower", "se_lower"):
        np.testing.assert_allclose(dev[key], lo[key], rtol=rtol, atol=rtol * K, err_msg=key)
    for key in ("upper", "se_upper"):
        np.testing.assert_allclose(dev[key], up[key], rtol=rtol, atol=rtol * K, err_msg=key)
    assert dev["ci_lo"] == dev["lower"] - 1.96 * dev["se_lower"] and dev["ci_hi"] == dev["upper"] + 1.96 * dev["se_upper"]
    assert (dev["n_lower"], dev["n_outer"], dev["n_inner"]) == (n_lower, n_outer, n_inner)
    return lo, up


# ---------------------------------------------------------------------------------------------- the device's own spots
def gbm_params(is_put=True, S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, N=8, M=4096, seed=42, stream=0):
    return _ffi.make_params(model="gbm", is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N, S0=S0, K=K, r=r, sigma=sigma,
                            T=T, seed=seed, stream=stream)


def gbm_fit_paths(ctx, p):
    return ctx.gbm_paths(int(p.n_paths), int(p.n_steps), p.S0, p.r, p.sigma, p.T, p.seed, p.stream, p.pair_offset)


def fit_paths(ctx, p):
    """the fitting paths of p, on the device"""
    if p.model == _ffi.MODELS["gbm"]:
        return gbm_fit_paths(ctx, p)
    return ctx.heston_paths(int(p.n_paths), int(p.n_steps), p.S0, p.r, p.T, *hc.hp_of(p), p.seed, p.stream, p.pair_offset,
                            int(p.heston_scheme))


def fitted_table(ctx, p, policy, k):
    """omc_lsm_poly's fits of semantics `policy` on the gathered matrix of p's fitting paths with horizon T_v, scattered to
    the scheduled rows of a table [N+1][4] (zero rows elsewhere); k < 2: the fits on the whole matrix"""
    N = int(p.n_steps)
    S = hc.host(fit_paths(ctx, p))
    G = ctx.to_device(gather(S, k))
    d = ctx.lsm_poly(G, p.K, p.r, horizon(p.T, N, k), bool(p.is_put), policy)
    G.free()
    t = np.zeros((N + 1, 4))
    rows = schedule(N, k)
    t[rows, :3], t[rows, 3] = d["betas"], d["nitm"]
    if int(k) >= 2:
        t[0] = 0.0
    return t


def given_table(ctx, p, holes=None):
    """a policy [N+1][4] from other paths (2048 of stream 9 of p's seed), textbook fits on every date, with n = 0 on the dates
    `holes` marks: the caller's table, NOT masked to a schedule"""
    q = type(p).from_buffer_copy(bytes(p))
    q.n_paths, q.stream, q.pair_offset = 2048, 9, 0
    t = fitted_table(ctx, q, "textbook", 0)
    if holes is not None:
        t[np.asarray(holes), 3] = 0.0
    return t


def device_spots(ctx, p, k, n_lower, n_outer, n_inner, streams=None):
    """-> dict Sl, So (and Vo under Heston) and inner(i, t) for the SCHEDULED t only: every item computed once, from the
    generators at the documented Philox coordinates (tests/test_gpu_bounds.py's `tiny` for GBM, heston_bounds_case.device_spots
    for Heston, with the inner cache built for tau_0 .. tau_{J-1} only)."""
    N = int(p.n_steps)
    ts = schedule(N, k)[:-1]
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    if p.model != _ffi.MODELS["gbm"]:
        sp = hc.device_spots(ctx, p, n_lower, n_outer, n_inner, streams=(s_lo, s_out, s_in))
        items = {(i, t): sp["inner"](i, t) for i in range(n_outer) for t in ts}
        return dict(Sl=sp["Sl"], So=sp["So"], Vo=sp["Vo"], inner=lambda i, t: items[(i, t)])
    Sl = hc.host(ctx.gbm_paths(n_lower, N, p.S0, p.r, p.sigma, p.T, p.seed, s_lo))
    So = hc.host(ctx.gbm_paths(n_outer, N, p.S0, p.r, p.sigma, p.T, p.seed, s_out))
    inner = br.inner_by_item(lambda off, n: hc.host(ctx.gbm_normals(n, N, p.seed, s_in, off)), So, n_inner,
                             lambda z, s0: hc.host(ctx.gbm_paths_from_normals(z, s0, p.r, p.sigma, p.T)))
    items = {(i, t): inner(i, t) for i in range(n_outer) for t in ts}
    return dict(Sl=Sl, So=So, inner=lambda i, t: items[(i, t)])


def price(ctx, p, **kw):
    """the bounds call of p's model"""
    if p.model == _ffi.MODELS["gbm"]:
        return ctx.price_american_bounds(p, **kw)
    return ctx.price_american_bounds_heston(p, **kw)


# ---------------------------------------------------------------------------------------------- the fuzz cases
MODELS = ("gbm", "heston0", "heston1")


def fuzz_cases(n, seed=20261020):
    """n seeded cases, as plain dicts: N in 1 .. 13, k in 0 .. N + 3 (every date, schedules with a short first gap, dates
    inside a Philox block, gaps longer than one, the expiry alone), n_inner of heston_bounds_case.N_INNER (a third and more
    with the refill), a ragged even n_outer, GBM and both Heston schemes (scheme 1 violating Feller on every other one), put /
    call, fitted policies and given tables with n = 0 holes, the float64 fallback on some."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        n_inner = hc.N_INNER[3 - c % 4] if c % 3 else int(rng.choice((130, 200)))
        N = int(rng.integers(1, 14))
        k = int(rng.integers(0, N + 4)) if c % 4 != 1 else int(rng.integers(2, max(3, N)))  # every fourth: a real schedule
        model = MODELS[c % 3]
        kappa, theta = float(rng.uniform(0.5, 4.0)), float(rng.uniform(0.01, 0.09))
        bound = float(np.sqrt(2.0 * kappa * theta))
        violate = model == "heston1" and (c // 3) % 2 == 0
        xi = bound * float(rng.uniform(1.3, 3.0)) if violate else bound * float(rng.uniform(0.2, 0.9))
        case = dict(N=N, k=k, n_inner=n_inner, n_outer=2 * int(rng.integers(1, 21)), n_lower=2 * int(rng.integers(100, 700)),
                    M=2 * int(rng.integers(300, 1500)), model=model, is_put=bool(rng.integers(0, 2)),
                    policy=hc.POLICIES[(c + c // 4) % 4], irr_every=int(rng.choice((0, 0, 1, 2, 3))),
                    seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)),
                    S0=100.0 * float(rng.uniform(0.8, 1.25)), K=100.0, r=float(rng.uniform(0.0, 0.08)),
                    T=float(rng.uniform(0.5, 3.0)), sigma=float(rng.uniform(0.1, 0.5)), v0=float(rng.uniform(0.01, 0.09)),
                    kappa=kappa, theta=theta, xi=xi, rho=float(rng.uniform(-0.9, 0.5)))
        case["feller"] = 2.0 * kappa * theta >= xi * xi
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]  # dates of a given table with n = 0
        case["refill"] = n_inner // 2 > 64
        case["J"] = n_dates(N, k)
        out.append(case)
    return out


def fuzz_params(case):
    if case["model"] == "gbm":
        return gbm_params(is_put=case["is_put"], S0=case["S0"], K=case["K"], r=case["r"], sigma=case["sigma"], T=case["T"],
                          N=case["N"], M=case["M"], seed=case["seed"], stream=case["stream"])
    return hc.make_params({key: case[key] for key in hc.HP_KEYS}, scheme=int(case["model"][-1]), is_put=case["is_put"],
                          S0=case["S0"], K=case["K"], r=case["r"], T=case["T"], N=case["N"], M=case["M"], seed=case["seed"],
                          stream=case["stream"])


def numpy_paths(case, rows, m, s0, seed):
    """float32 log-normal paths [rows][m] from s0 on the case's grid (antithetic layout): what the CPU test restates a case on"""
    rng = np.random.default_rng(seed)
    dt = case["T"] / case["N"]
    sig = case["sigma"]
    z = rng.standard_normal((rows - 1, m // 2))
    z = np.concatenate([z, -z], axis=1)
    x = np.cumsum((case["r"] - 0.5 * sig * sig) * dt + sig * math.sqrt(dt) * z, axis=0)
    return np.concatenate([np.full((1, m), s0), s0 * np.exp(x)]).astype(np.float32)

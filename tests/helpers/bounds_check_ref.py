"""numpy restatement of the price bounds with sub-optimality checking (option "bounds_suboptimality" = m; the rule is in
DESIGN.md section 27 and include/omc.h), built on tests/helpers/bounds_ref.py and bounds_cv_ref.py.  TEST INFRASTRUCTURE ONLY.

With s = So[t][i] (float32), x = float64(s), phi(x) = K - x (put) or x - K (call), item (i, t), 0 <= t < N, is KEPT iff
    t == 0,   or the policy stops at (s, t) (bounds_ref.stop_rule),
    or m == 1 and phi(x) > 0,   or m == 2 and phi(x) > E(x, t) (bounds_cv_ref.euro).
Inner simulations run at kept items only -- their Q^ is the unchecked call's, a skipped item's entry is 0.0, the step count is
the kept items' -- and the walk visits the kept dates and N:  M = 0, lq = Q^_0;  L = Z_t where the policy stops (and at N),
else Q^_t (Q^_N = 0);  M = M + L - lq;  candidate Z_t - M;  lq = Q^_t.  The sample is the largest candidate.
"""
from __future__ import annotations

import math

import numpy as np

from helpers import bounds_cv_ref as cv
from helpers import bounds_ref as br

MODES = ("off", "payoff", "european")
BORDER = 1e-9  # |phi - E| <= BORDER K: a mode-2 item whose decision libm and the device's erfc / log may make differently


def keep(So, betas4, m, K, r, T, is_put, sigma=None):
    """-> dict keep [N][n_outer] bool (keep[t][i]: date-major as So), ties (stop decisions within bounds_ref.TIE K of the
    continuation value), borderline (mode 2: items not kept by t == 0 or a stop with |phi - E| <= BORDER K)"""
    N, n = So.shape[0] - 1, So.shape[1]
    kp = np.zeros((N, n), bool)
    if N > 0:
        kp[0] = True
    ties = borderline = 0
    for t in range(1, N):
        st, ti = br.stop_rule(So[t], t, N, K, is_put, betas4)
        ties += ti
        x = So[t].astype(np.float64)
        phi = (K - x) if is_put else (x - K)
        if m == 0:
            kp[t] = True
        elif m == 1:
            kp[t] = st | (phi > 0.0)
        else:
            E = cv.euro(So[t], t, N, K, r, sigma, T, is_put)
            kp[t] = st | ~(phi <= E)  # phi > E, or a NaN
            borderline += int(np.count_nonzero(~st & (np.abs(phi - E) <= BORDER * K)))
    return dict(keep=kp, ties=ties, borderline=borderline)


def item_steps(So, inner, rows, K, r, T, is_put, betas4):
    """the plain Q^ (bounds_ref.q_rows' values) and the inner path steps of EVERY item of the outer paths in `rows` -> dict q
    [len(rows)][N], steps [len(rows)][N] int64, ties"""
    N = So.shape[0] - 1
    q = np.zeros((len(rows), N))
    steps = np.zeros((len(rows), N), np.int64)
    ties = 0
    for k, i in enumerate(rows):
        for t in range(N):
            tau, Z, ti = br.first_stop(inner(i, t), t, N, K, r, T, is_put, betas4)
            q[k, t] = Z.sum() / Z.size
            steps[k, t] = int((tau - t).sum())
            ties += ti
    return dict(q=q, steps=steps, ties=ties)


def q_rows(So, inner, rows, kp, K, r, T, is_put, betas4, sigma=None):
    """Q^ of the KEPT items of the outer paths in `rows` (sigma given: the controlled estimator of bounds_cv_ref) -> dict q
    [len(rows)][N] (0.0 at skipped items), inner_path_steps (the kept items'), ties"""
    N = So.shape[0] - 1
    D = cv.discounts(N, r, T)
    q = np.zeros((len(rows), N))
    steps = ties = 0
    for k, i in enumerate(rows):
        for t in range(N):
            if not kp[t, i]:
                continue
            if sigma is None:
                tau, Z, ti = br.first_stop(inner(i, t), t, N, K, r, T, is_put, betas4)
                q[k, t] = Z.sum() / Z.size
            else:
                tau, x, Z, ti = cv.stopped(inner(i, t), t, N, K, r, T, is_put, betas4)
                c = cv.terms(tau, x, Z, N, K, r, sigma, T, is_put)
                q[k, t] = D[t] * float(cv.euro(So[t, i], t, N, K, r, sigma, T, is_put)) + math.fsum(c) / c.size
            steps += int((tau - t).sum())
            ties += ti
    return dict(q=q, inner_path_steps=steps, ties=ties)


def walk_rows(So, q, rows, kp, K, r, T, is_put, betas4):
    """The walk over the kept dates and N of the outer paths in `rows` with their Q^ q [len(rows)][N] -> dict samples
    [len(rows)], M [len(rows)][N+1] (the martingale at the visited dates, NaN elsewhere, M[:, 0] = 0), ties, zmax"""
    N = So.shape[0] - 1
    D = cv.discounts(N, r, T)
    samples = np.zeros(len(rows))
    Ms = np.full((len(rows), N + 1), np.nan)
    ties = 0
    zmax = 0.0
    for k, i in enumerate(rows):
        M, best, lq = 0.0, -math.inf, q[k, 0] if N > 0 else 0.0
        Ms[k, 0] = 0.0
        for t in range(1, N + 1):
            if t < N and not kp[t, i]:
                continue
            s = So[t, i:i + 1]
            phi = (K - float(s[0])) if is_put else (float(s[0]) - K)
            Zt = D[t] * max(phi, 0.0)
            zmax = max(zmax, Zt)
            st, ti = br.stop_rule(s, t, N, K, is_put, betas4)
            ties += ti
            qt = q[k, t] if t < N else 0.0
            L = Zt if st[0] else qt
            M = M + L - lq
            Ms[k, t] = M
            best = max(best, Zt - M)
            lq = qt
        samples[k] = best
    return dict(samples=samples, M=Ms, ties=ties, zmax=zmax)


def upper_bound(So, inner, m, K, r, T, is_put, betas4, sigma=None, cv_sigma=None):
    """the checked upper bound on the restatement: sigma is E's volatility (mode 2), cv_sigma that of the control variate
    (None: the plain estimator) -> dict upper, se_upper, q, samples, keep, inner_path_steps, ties, borderline, zmax"""
    rows = range(So.shape[1])
    kd = keep(So, betas4, m, K, r, T, is_put, sigma)
    qr = q_rows(So, inner, rows, kd["keep"], K, r, T, is_put, betas4, cv_sigma)
    wk = walk_rows(So, qr["q"], rows, kd["keep"], K, r, T, is_put, betas4)
    up, se, _ = br._pair_mean_se(wk["samples"])
    return dict(upper=up, se_upper=se, q=qr["q"], samples=wk["samples"], M=wk["M"], keep=kd["keep"],
                inner_path_steps=qr["inner_path_steps"], ties=kd["ties"] + qr["ties"] + wk["ties"],
                borderline=kd["borderline"], zmax=wk["zmax"])


# ---------------------------------------------------------------------------------------------- the fuzz cases
FUZZ_MODELS = ("gbm", "gbm-cv", "basket", "asian", "heston1")


def fuzz_cases(n, seed=20261022):
    """n seeded cases, as plain dicts: every model that takes a check, mode 2 on the GBM ones, N in 1 .. 13, n_inner over every
    lane group, a ragged group and the refill, a ragged even n_outer, put / call, fitted policies and given tables with n = 0
    holes, the float64 fallback on some.  The spot starts near the strike, so that every mode skips and keeps."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        model = FUZZ_MODELS[c % 5]
        N = int(rng.integers(1, 14))
        case = dict(N=N, model=model, mode=(2 if model.startswith("gbm") and c % 2 == 0 else 1),
                    n_inner=(16, 2, 64, 24, 192, 130, 10, 66)[c % 8], n_outer=2 * int(rng.integers(2, 17)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy=("textbook", "given", "two_pass", "reference")[(c + c // 4) % 4],
                    irr_every=int(rng.choice((0, 0, 1, 2, 3))), seed=int(rng.integers(1, 1 << 31)),
                    stream=int(rng.integers(0, 50)), S0=100.0 * float(rng.uniform(0.9, 1.1)), K=100.0,
                    r=float(rng.uniform(0.0, 0.08)), T=float(rng.uniform(0.5, 3.0)), sigma=float(rng.uniform(0.1, 0.5)))
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]
        out.append(case)
    return out


# ---------------------------------------------------------------------------------------------- the device's calls and spots
# model keys: "gbm", "gbm-cv" (the control variate on), "basket" / "asian" (two assets, a policy on the index), "heston0" /
# "heston1" (a policy on the spot).  The imports are local: the CPU tests above need none of them.
WALK_RTOL = 1e-12  # the device's walk against a float64 walk on the same Q^ (tests/test_gpu_bounds.py: rtol, atol rtol K)


def basket_of(model, S0):
    from options_model_amd import _ffi
    return _ffi.make_basket([S0 - 4.0, S0 + 3.0], [0.16, 0.22], [0.0, 0.03], [0.5, 0.5], np.array([[1.0, -0.4], [-0.4, 1.0]]),
                            "asian" if model == "asian" else "basket")


def params_of(model, is_put=True, S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, N=8, M=4096, seed=42, stream=0, hp=None):
    """-> (params, basket or None)"""
    from helpers import bounds_schedule_ref as bs
    from helpers import heston_bounds_case as hc
    if model.startswith("heston"):
        return hc.make_params(hp or hc.HP, scheme=int(model[-1]), is_put=is_put, S0=S0, K=K, r=r, T=T, N=N, M=M, seed=seed,
                              stream=stream), None
    p = bs.gbm_params(is_put=is_put, S0=S0, K=K, r=r, sigma=sigma, T=T, N=N, M=M, seed=seed, stream=stream)
    return p, (basket_of(model, S0) if model in ("basket", "asian") else None)


def call(ctx, model, p, b, mode, **kw):
    """the bounds call of the model with sub-optimality check MODES[mode] (None: the option as the context holds it)"""
    chk = None if mode is None else MODES[mode]
    if model in ("gbm", "gbm-cv"):
        return ctx.price_american_bounds(p, control_variate=model == "gbm-cv", suboptimality_check=chk, **kw)
    if model in ("basket", "asian"):
        return ctx.price_american_basket_bounds(p, b, suboptimality_check=chk, **kw)
    return ctx.price_american_bounds_heston(p, suboptimality_check=chk, **kw)


def given_table(ctx, model, p, b, holes=None, scale_call=0.9):
    """a table [N+1][4] that does stop paths early: textbook fits on other paths; for a call (never exercised early without
    dividends) with the continuation values scaled down"""
    from helpers import asian_ref as ar
    from helpers import basket_bounds_case as bc
    from helpers import bounds_schedule_ref as bs
    if model == "asian":
        t = ar.given_table4(ctx, p, b, holes)
    elif model == "basket":
        t = bc.fitted_table(ctx, bc.with_fields(p, n_paths=2048, stream=9, pair_offset=0), b, "textbook")
        if holes is not None:
            t[np.asarray(holes), 3] = 0.0
    else:
        t = bs.given_table(ctx, p, holes)
    if not p.is_put:
        t[:, :3] *= scale_call
    return t


def device_spots(ctx, model, p, b, n_lower, n_outer, n_inner):
    """the device's own outer index matrix So [N+1][n_outer] and inner(i, t) -> the index spots of the item's inner paths
    [N - t + 1][n_inner]; free() releases what the builders keep on the device"""
    from helpers import asian_ref as ar
    from helpers import basket_bounds_case as bc
    from helpers import bounds_schedule_ref as bs
    from helpers import heston_bounds_case as hc
    if model == "asian":
        sp = ar.device_spots(ctx, p, b, n_lower, n_outer, n_inner)
        return dict(So=sp["Xo"], inner=lambda i, t: sp["inner"](i, t)[0], free=sp["free"])
    if model == "basket":
        sp = bc.device_spots(ctx, p, b, n_lower, n_outer, n_inner)
        return dict(So=sp["So"], inner=sp["inner"], free=sp["free"])
    if model.startswith("heston"):
        sp = hc.device_spots(ctx, p, 2, n_outer, n_inner)
        return dict(So=sp["So"], inner=sp["inner"], free=lambda: None)
    N = int(p.n_steps)
    So = hc.host(ctx.gbm_paths(n_outer, N, p.S0, p.r, p.sigma, p.T, p.seed, p.stream + 2))
    inner = br.inner_by_item(lambda off, n: hc.host(ctx.gbm_normals(n, N, p.seed, p.stream + 3, off)), So, n_inner,
                             lambda z, s0: hc.host(ctx.gbm_paths_from_normals(z, s0, p.r, p.sigma, p.T)))
    return dict(So=So, inner=inner, free=lambda: None)


def outer_index(ctx, model, p, b, n_outer):
    """So alone, for the tests that restate no inner path"""
    from helpers import basket_bounds_case as bc
    from helpers import heston_bounds_case as hc
    N = int(p.n_steps)
    if model in ("basket", "asian"):
        return bc.index_and_assets(ctx, bc.with_fields(p, n_paths=n_outer, stream=p.stream + 2, pair_offset=0), b, assets=False)[0]
    if model.startswith("heston"):
        Sd, Vd = ctx.heston_paths_sv(n_outer, N, p.S0, p.r, p.T, *hc.hp_of(p), p.seed, p.stream + 2, 0, int(p.heston_scheme))
        Vd.free()
        return hc.host(Sd)
    return hc.host(ctx.gbm_paths(n_outer, N, p.S0, p.r, p.sigma, p.T, p.seed, p.stream + 2))


def check_against_dense(p, dense, got, mode, So, sigma=None, steps=None, rows=None):
    """The device's checked call `got` (want_q, want_samples) against its dense call `dense` and the restatement on the device's
    own outer index So: the same policy and lower bound, bit for bit; no stop tie and no borderline item; Q^ the dense call's
    bits at the kept items and 0.0 at the skipped ones; the samples equal to this file's walk on the device's Q^ and at most the
    dense ones; with `steps` (item_steps(...)["steps"] of every item) the dense and the kept step counts.  rows: the outer paths whose walk is restated (None: all, and the upper bound with them).
    -> the keep mask"""
    K, is_put, N = float(p.K), bool(p.is_put), int(p.n_steps)
    np.testing.assert_array_equal(got["betas"], dense["betas"])
    for key in ("lower", "se_lower", "n_exercised_lower", "ci_lo", "n_lower", "n_outer", "n_inner"):
        assert got[key] == dense[key], key
    kd = keep(So, got["betas"], mode, K, p.r, p.T, is_put, sigma)
    assert kd["ties"] == 0 and kd["borderline"] == 0  # numpy's decisions are the device's
    kp = kd["keep"].T  # [n_outer][N] as q
    np.testing.assert_array_equal(got["q"][kp], dense["q"][kp])
    assert np.all(got["q"][~kp] == 0.0) and not np.signbit(got["q"][~kp]).any()
    sampled = rows is not None
    rows = list(rows) if sampled else list(range(So.shape[1]))
    wk = walk_rows(So, got["q"][rows], rows, kd["keep"], K, p.r, p.T, is_put, got["betas"])
    assert wk["ties"] == 0
    np.testing.assert_allclose(got["samples"][rows], wk["samples"], rtol=WALK_RTOL, atol=WALK_RTOL * K)
    assert np.all(got["samples"] <= dense["samples"] + br.samples_atol(N, dense["q"], K) + WALK_RTOL * K)
    if not sampled:
        up, se, ratio = br._pair_mean_se(wk["samples"])
        np.testing.assert_allclose(got["upper"], up, rtol=WALK_RTOL, atol=WALK_RTOL * K)
        # (beside the walk's tolerance, what the device's own E[m^2] - mean^2 loses to cancellation: bounds_cv_ref.se_atol)
        assert abs(got["se_upper"] - se) <= WALK_RTOL * K + cv.se_atol(se, ratio, up, So.shape[1] // 2)
    assert got["ci_hi"] == got["upper"] + 1.96 * got["se_upper"]
    if steps is not None:
        assert dense["inner_path_steps"] == int(steps.sum())
        assert got["inner_path_steps"] == int(steps[kp].sum())
    else:
        assert got["inner_path_steps"] <= dense["inner_path_steps"]
    return kd["keep"]

"""numpy restatement of the price bounds whose policy sees the index and the runner-up
(omc_price_american_basket_bounds_runnerup; the definitions are in include/omc.h and DESIGN.md section 18).  TEST
INFRASTRUCTURE ONLY.

bounds_ref.py with pairs (X, Y) in the place of the spot: X the index, Y the second order statistic of the weighted spots
v_k = w_k s_k (float32 products), both formed here from the device's own ASSET matrices -- X is asserted to have the bits of
the device's index matrix.  The policy betas8 [N+1][8] = (c0 .. c5, n, 0): at 1 <= t < N a path exercises iff n > 0.5,
imm = phi(X) > 0 and imm > c0 + c1 u + c2 u^2 + c3 w + c4 w^2 + c5 u w (u = X / K - 1, w = Y / K - 1); at N it takes its
payoff.  numpy has no fused multiply-add, so a decision within TIE * K of the continuation value counts as a tie (bounds_ref.TIE):
where there are none, the decisions are the device's.  The spots come from omc_price_american_basket calls at the documented
Philox coordinates, as helpers/basket_bounds_case.py describes; the restart call of an inner item keeps its assets too.
Also: the Longstaff-Schwartz fit of one date (the centred LDL' solve with the truncation rule) and its date-by-date check
against the device's table, and the seeded cases of tests/test_gpu_runnerup_bounds_fuzz.py, which need no GPU.
"""
from __future__ import annotations

import math

import numpy as np

from helpers import basket_bounds_case as bc
from helpers import bounds_ref as br
from options_model_amd import _ffi

KINDS = ("best-of", "worst-of")
POLICIES = ("textbook", "given")
REG = "index+runner-up"


# ---------------------------------------------------------------------------------------------- the regressors
def xy(A, w, kind, S=None):
    """Asset spots A [d][...] float32, weights w [d], kind -> (X, Y) float32 [...] by the float32 rule.  S: the device's
    index spots of the same paths; X must have their bits."""
    A = np.asarray(A, np.float32)
    if A.shape[0] < 2:
        raise ValueError("the runner-up needs two assets")
    wf = np.asarray(w, np.float64).astype(np.float32).reshape((-1,) + (1,) * (A.ndim - 1))
    v = np.sort(wf * A, axis=0)  # float32 products; order statistics are values, no order of evaluation
    X, Y = (v[-1], v[-2]) if kind == "best-of" else (v[0], v[1])
    if S is not None:
        np.testing.assert_array_equal(X.view(np.uint32), np.asarray(S, np.float32).view(np.uint32))
    return X, Y


def basket_weights(b):
    return [float(b.w[k]) for k in range(int(b.n_assets))]


def basket_kind(b):
    return {v: k for k, v in _ffi.BASKET_KINDS.items() if k in KINDS}[int(b.kind)]


def uw(X, Y, K):
    return X.astype(np.float64) * (1.0 / K) - 1.0, Y.astype(np.float64) * (1.0 / K) - 1.0


def continuation(u, w, row):
    c0, c1, c2, c3, c4, c5 = (float(x) for x in row[:6])
    return w * (w * c4 + (u * c5 + c3)) + (u * (u * c2 + c1) + c0)


# ---------------------------------------------------------------------------------------------- the two estimators
def stop_rule(X, Y, t, N, K, is_put, betas8):
    """-> (stops [bool], ties [int]) for float32 pairs (X, Y) at date t."""
    if t >= N:
        return np.ones(X.shape, bool), 0
    if not betas8[t][6] > 0.5:
        return np.zeros(X.shape, bool), 0
    xd = X.astype(np.float64)
    imm = K - xd if is_put else xd - K
    cont = continuation(*uw(X, Y, K), betas8[t])
    itm = imm > 0.0
    return itm & (imm > cont), int(np.count_nonzero(itm & (np.abs(imm - cont) <= br.TIE * K)))


def first_stop(X, Y, t0, N, K, r, T, is_put, betas8):
    """Paths X, Y [N - t0 + 1][m] (row k = date t0 + k): tau = first date > t0 where the rule fires -> (tau, x at tau, Z,
    ties)."""
    m = X.shape[1]
    tau = np.full(m, -1, np.int64)
    x = np.zeros(m, np.float32)
    ties = 0
    for k in range(1, N - t0 + 1):
        st, ti = stop_rule(X[k], Y[k], t0 + k, N, K, is_put, betas8)
        ties += ti if k + t0 < N else 0
        ex = (tau < 0) & st
        tau[ex] = t0 + k
        x[ex] = X[k][ex]
    phi = (K - x.astype(np.float64)) if is_put else (x.astype(np.float64) - K)
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    return tau, x, D[tau] * np.maximum(phi, 0.0), ties


def lower_bound(X, Y, K, r, T, is_put, betas8):
    """X, Y: the lower-bound paths [N+1][n_lower] (antithetic layout) -> dict as bounds_ref.lower_bound."""
    N = X.shape[0] - 1
    tau, _, Z, ties = first_stop(X, Y, 0, N, K, r, T, is_put, betas8)
    lo, se, ratio = br._pair_mean_se(Z)
    return dict(lower=lo, se_lower=se, se_cancel=ratio, n_exercised=int(np.count_nonzero(tau < N)), ties=ties)


def q_rows(N, inner, rows, K, r, T, is_put, betas8):
    """Q^_t[i] for the outer paths i in `rows`, all dates -> dict q [len(rows)][N], inner_path_steps, ties.  inner(i, t) ->
    (X, Y) of the item's inner paths, each [N - t + 1][n_inner]."""
    q = np.zeros((len(rows), N))
    steps = ties = 0
    for k, i in enumerate(rows):
        for t in range(N):
            Xi, Yi = inner(i, t)
            tau, _, Z, ti = first_stop(Xi, Yi, t, N, K, r, T, is_put, betas8)
            q[k, t] = Z.sum() / Z.size
            steps += int((tau - t).sum())
            ties += ti
    return dict(q=q, inner_path_steps=steps, ties=ties)


def walk_rows(Xo, Yo, q, rows, K, r, T, is_put, betas8):
    """The martingale walk of the outer paths in `rows` with their Q^ -> dict samples, ties, zmax (bounds_ref.walk_rows)."""
    N = Xo.shape[0] - 1
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    samples = np.zeros(len(rows))
    ties = 0
    zmax = 0.0
    for k, i in enumerate(rows):
        M, best = 0.0, -math.inf
        for t in range(1, N + 1):
            x = Xo[t, i:i + 1]
            phi = (K - float(x[0])) if is_put else (float(x[0]) - K)
            Zt = D[t] * max(phi, 0.0)
            zmax = max(zmax, Zt)
            st, ti = stop_rule(x, Yo[t, i:i + 1], t, N, K, is_put, betas8)
            ties += ti
            qt = q[k, t] if t < N else 0.0
            M = M + (Zt if st[0] else qt) - q[k, t - 1]
            best = max(best, Zt - M)
        samples[k] = best
    return dict(samples=samples, ties=ties, zmax=zmax)


def upper_bound(Xo, Yo, inner, K, r, T, is_put, betas8):
    rows = range(Xo.shape[1])
    qr = q_rows(Xo.shape[0] - 1, inner, rows, K, r, T, is_put, betas8)
    wk = walk_rows(Xo, Yo, qr["q"], rows, K, r, T, is_put, betas8)
    up, se, ratio = br._pair_mean_se(wk["samples"])
    return dict(upper=up, se_upper=se, se_cancel=ratio, q=qr["q"], samples=wk["samples"],
                inner_path_steps=qr["inner_path_steps"], ties=qr["ties"] + wk["ties"], zmax=wk["zmax"])


# ---------------------------------------------------------------------------------------------- the device's own spots
def paths_xy(ctx, p, b):
    """(X, Y) [N+1][n_paths] of omc_price_american_basket(p, b), X checked against its index matrix"""
    S, A = bc.index_and_assets(ctx, p, b)
    return xy(A, basket_weights(b), basket_kind(b), S)


def device_spots(ctx, p, b, n_lower, n_outer, n_inner, streams=None, lower=True):
    """-> dict Xl, Yl (lower paths), Xo, Yo (outer paths) and inner(i, t) -> (X, Y) [N - t + 1][n_inner]: the index and the
    assets of the restart call basket_bounds_case.device_spots describes"""
    N, d = int(p.n_steps), int(b.n_assets)
    w, kind = basket_weights(b), basket_kind(b)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Xl, Yl = paths_xy(ctx, bc.with_fields(p, n_paths=n_lower, stream=s_lo, pair_offset=0), b) if lower else (None, None)
    So, Ao = bc.index_and_assets(ctx, bc.with_fields(p, n_paths=n_outer, stream=s_out, pair_offset=0), b)
    Xo, Yo = xy(Ao, w, kind, So)
    H = n_inner // 2
    keep = ctx.empty((N + 1, n_inner), np.float32)
    akeep = ctx.empty((d, N + 1, n_inner), np.float32)

    def inner(i, t):
        rb = bc.with_fields(b)
        for k in range(d):
            rb.S0[k] = float(Ao[k, t, i])
        ctx.price_american_basket(bc.with_fields(p, n_paths=n_inner, stream=s_in, pair_offset=(i * (N + 1) + t) * H), rb,
                                  S_keep=keep, assets_keep=akeep)
        return xy(akeep.to_host()[:, :N - t + 1], w, kind, keep.to_host()[:N - t + 1])

    def free():
        keep.free()
        akeep.free()

    return dict(Xl=Xl, Yl=Yl, Xo=Xo, Yo=Yo, inner=inner, free=free)


def check_against_restatement(ctx, p, b, dev, n_lower, n_outer, n_inner, rtol=1e-12):
    """basket_bounds_case.check_against_restatement for the two-regressor policy dev["betas"] [N+1][8]"""
    K, is_put = float(p.K), bool(p.is_put)
    sp = device_spots(ctx, p, b, n_lower, n_outer, n_inner)
    try:
        lo = lower_bound(sp["Xl"], sp["Yl"], K, p.r, p.T, is_put, dev["betas"])
        up = upper_bound(sp["Xo"], sp["Yo"], sp["inner"], K, p.r, p.T, is_put, dev["betas"])
    finally:
        sp["free"]()
    assert lo["ties"] == 0 and up["ties"] == 0  # numpy's decisions are the device's
    assert dev["n_exercised_lower"] == lo["n_exercised"]
    assert dev["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(dev["q"], up["q"], rtol=rtol, atol=rtol * K)
    np.testing.assert_allclose(dev["samples"], up["samples"], rtol=rtol, atol=rtol * K)
    for k in ("lower", "se_lower"):
        np.testing.assert_allclose(dev[k], lo[k], rtol=rtol, atol=rtol * K, err_msg=k)
    for k in ("upper", "se_upper"):
        np.testing.assert_allclose(dev[k], up[k], rtol=rtol, atol=rtol * K, err_msg=k)
    assert dev["ci_lo"] == dev["lower"] - 1.96 * dev["se_lower"] and dev["ci_hi"] == dev["upper"] + 1.96 * dev["se_upper"]
    assert (dev["n_lower"], dev["n_outer"], dev["n_inner"]) == (n_lower, n_outer, n_inner)
    return lo, up


# ---------------------------------------------------------------------------------------------- the fit
def ldl_fit(u, w, y):
    """The policy row (c0 .. c5, n, 0) of one date from its regression set: features f = (u, u^2, w, w^2, uw), the centred
    system solved by LDL' without pivoting in the order of f; feature j (from 0) and every later one get coefficient 0
    when n < j + 1.5 or the pivot is not above 1e-12 |C_jj| + 1e-300."""
    row = np.zeros(8)
    n = int(u.size)
    if n == 0:
        return row
    F = np.stack([u, u * u, w, w * w, u * w])
    sf = np.array([math.fsum(f) for f in F])
    sy = math.fsum(y)
    fbar, ybar = sf / n, sy / n
    C = np.array([[math.fsum(F[a] * F[b]) - sf[a] * fbar[b] for b in range(5)] for a in range(5)])
    c = np.array([math.fsum(F[a] * y) - sf[a] * ybar for a in range(5)])
    L, dd, kept = np.zeros((5, 5)), np.zeros(5), 0
    for j in range(5):
        for i in range(j):
            L[j, i] = (C[j, i] - sum(L[j, m] * L[i, m] * dd[m] for m in range(i))) / dd[i]
        piv = C[j, j] - sum(L[j, m] * L[j, m] * dd[m] for m in range(j))
        if n < j + 1.5 or not piv > 1e-12 * abs(C[j, j]) + 1e-300:
            break
        dd[j], kept = piv, j + 1
    z, x = np.zeros(5), np.zeros(5)
    for j in range(kept):
        z[j] = c[j] - sum(L[j, m] * z[m] for m in range(j))
    for j in range(kept - 1, -1, -1):
        x[j] = z[j] / dd[j] - sum(L[m, j] * x[m] for m in range(j + 1, kept))
    row[0] = ybar - float(x @ fbar)
    row[1:6] = x
    row[6] = n
    return row


def check_fit(X, Y, K, r, T, is_put, betas8, tol=1e-9):
    """The device's fitted table betas8 on its own fitting paths (X, Y) [N+1][M], date by date: for t = N-1 .. 1 the later
    dates are decided with the DEVICE's rows (no ties), the date's regression set and targets formed, the row solved here;
    the two continuation values on the set agree within tol * K and n_t is equal.  -> the largest difference / K."""
    N = X.shape[0] - 1
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    assert not betas8[0].any() and not betas8[N].any()
    worst = 0.0
    for t in range(N - 1, 0, -1):
        tau, x_ex, _, ties = first_stop(X[t:], Y[t:], t, N, K, r, T, is_put, betas8)
        assert ties == 0, (t, ties)
        xd = X[t].astype(np.float64)
        itm = (K - xd if is_put else xd - K) > 0.0
        xe = x_ex[itm].astype(np.float64)
        y = D[tau[itm] - t] * np.maximum(K - xe if is_put else xe - K, 0.0)
        u, w = uw(X[t][itm], Y[t][itm], K)
        row = ldl_fit(u, w, y)
        assert betas8[t][6] == row[6] == np.count_nonzero(itm), (t, betas8[t][6], row[6])
        assert betas8[t][7] == 0.0
        if row[6] > 0:
            diff = float(np.max(np.abs(continuation(u, w, betas8[t]) - continuation(u, w, row))))
            assert diff <= tol * K, (t, diff)
            worst = max(worst, diff / K)
        else:
            assert not betas8[t].any()
    return worst


# ---------------------------------------------------------------------------------------------- the fuzz cases
N_INNER = (2, 64, 130, 200)


def fuzz_cases(n, seed=20261018):
    """n seeded cases of the fuzz sweep, as plain dicts: d in 2 .. 8 cycled and both kinds, N in 1 .. 13, n_inner of N_INNER
    (at least a third with more inner pairs than a wave has lanes: the refill), a ragged n_outer, put / call; every third
    case a given table with n = 0 holes, the others fitted."""
    rng = np.random.default_rng(seed)
    perm_d = rng.permutation(7)
    out = []
    for c in range(n):
        d = int(perm_d[c % 7]) + 2
        kind = KINDS[(c + c // 2) % 2]
        n_inner = N_INNER[3 - c % 4] if c % 3 else int(rng.choice((130, 200)))
        N = int(rng.integers(1, 14))
        case = dict(d=d, kind=kind, N=N, n_inner=n_inner, n_outer=2 * int(rng.integers(1, 12)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy="given" if c % 3 == 2 else "textbook",
                    seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)),
                    S0=[float(x) for x in rng.uniform(85.0, 115.0, d)], sigma=[float(x) for x in rng.uniform(0.1, 0.4, d)],
                    q=[float(x) for x in rng.uniform(0.0, 0.08, d)], rho=bc.random_correlation(rng, d),
                    T=float(rng.uniform(0.5, 3.0)))
        w = rng.uniform(0.5, 1.5, d)
        case["w"] = [float(x) for x in w / w.mean()]
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]  # dates of a given table with n = 0
        case["refill"] = n_inner // 2 > 64
        out.append(case)
    return out


def given_table(ctx, p, b, holes=None):
    """a two-regressor policy from other paths (2048 of stream 9 of p's seed), with n = 0 on the dates `holes` marks"""
    d = ctx.price_american_basket_bounds(bc.with_fields(p, n_paths=2048, stream=9, pair_offset=0), b, policy="textbook",
                                         n_lower=2, n_outer=2, n_inner=2, regressors=REG)
    t = d["betas"].copy()
    if holes is not None:
        t[np.asarray(holes), 6] = 0.0
    return t

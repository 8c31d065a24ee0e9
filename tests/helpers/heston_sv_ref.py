"""numpy restatement of the Heston price bounds whose policy sees the spot and the variance state
(omc_price_american_bounds_heston with cfg.regressors = 1; the definitions are in include/omc.h and DESIGN.md section 21).
TEST INFRASTRUCTURE ONLY.

runnerup_ref.py with (X, Y) = (spot, variance state) and w scaled by 1 / vbar, vbar = max(v0, theta), in the place of 1 / K.
The policy betas8 [N+1][8] = (c0 .. c5, n, 0): at 1 <= t < N a path exercises iff n > 0.5, imm = phi(X) > 0 and
imm > c0 + c1 u + c2 u^2 + c3 w + c4 w^2 + c5 u w (u = X / K - 1, w = Y / vbar - 1); at N it takes its payoff.  numpy has no
fused multiply-add, so a decision within TIE * K of the continuation value counts as a tie (bounds_ref.TIE): where there are
none, the decisions are the device's.  The fit of one date is runnerup_ref.ldl_fit (the same centred LDL' and truncation rule).

The device's own states come from the generator that keeps the variance, at the documented Philox coordinates:
  fitting paths  Context.heston_paths_sv(n_paths, ..) at (seed, stream, pair_offset)
  lower paths    ... (n_lower, ..) at stream_lower, pair_offset 0
  outer paths    ... (n_outer, ..) at stream_outer, pair_offset 0: So, Vo
  inner paths    of item (i, t): ... (n_inner, N, S0 = So[t, i], v0 = Vo[t, i], ..) at stream_inner, pair_offset
                 (i (N+1) + t) n_inner / 2, rows 0 .. N-t: step k of that call consumes the pair's Heston step k, as the inner
                 kernel does, and a float32 is exact in the double arguments.
With scheme 1 (full truncation) the outer states are negative now and then, and the generator takes such a v0 as it is.
Also the seeded cases of tests/test_gpu_heston_sv_bounds_fuzz.py and a float32 numpy Heston generator for them, which need no
GPU (test_heston_sv_bounds_cpu.py).
"""
from __future__ import annotations

import math

import numpy as np

from helpers import bounds_ref as br
from helpers import heston_bounds_case as hc
from helpers import runnerup_ref as rr

REG = "spot+variance"
POLICIES = ("textbook", "given")
f32 = np.float32


def vbar_of(p):
    return max(float(p.v0), float(p.theta))


# ---------------------------------------------------------------------------------------------- the rule
def uw(X, Y, K, vbar):
    return X.astype(np.float64) * (1.0 / K) - 1.0, Y.astype(np.float64) * (1.0 / vbar) - 1.0


def stop_rule(X, Y, t, N, K, is_put, betas8, vbar):
    """-> (stops [bool], ties [int]) for float32 pairs (X, Y) = (spot, variance state) at date t."""
    if t >= N:
        return np.ones(X.shape, bool), 0
    row = betas8[t]
    if not row[6] > 0.5:
        return np.zeros(X.shape, bool), 0
    xd = X.astype(np.float64)
    imm = K - xd if is_put else xd - K
    u, w = uw(X, Y, K, vbar)
    cont = rr.continuation(u, w, row)
    itm = imm > 0.0
    return itm & (imm > cont), int(np.count_nonzero(itm & (np.abs(imm - cont) <= br.TIE * K)))


def first_stop(X, Y, t0, N, K, r, T, is_put, betas8, vbar):
    """Paths X, Y [N - t0 + 1][m] (row k = date t0 + k): tau = first date > t0 where the rule fires -> (tau, x at tau, Z,
    ties)."""
    m = X.shape[1]
    tau = np.full(m, -1, np.int64)
    x = np.zeros(m, np.float32)
    ties = 0
    for k in range(1, N - t0 + 1):
        st, ti = stop_rule(X[k], Y[k], t0 + k, N, K, is_put, betas8, vbar)
        ties += ti if k + t0 < N else 0
        ex = (tau < 0) & st
        tau[ex] = t0 + k
        x[ex] = X[k][ex]
    phi = (K - x.astype(np.float64)) if is_put else (x.astype(np.float64) - K)
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    return tau, x, D[tau] * np.maximum(phi, 0.0), ties


def lower_bound(X, Y, K, r, T, is_put, betas8, vbar):
    """X, Y: the lower-bound paths [N+1][n_lower] (antithetic layout) -> dict as bounds_ref.lower_bound."""
    N = X.shape[0] - 1
    tau, _, Z, ties = first_stop(X, Y, 0, N, K, r, T, is_put, betas8, vbar)
    lo, se, ratio = br._pair_mean_se(Z)
    return dict(lower=lo, se_lower=se, se_cancel=ratio, n_exercised=int(np.count_nonzero(tau < N)), ties=ties)


def q_rows(N, inner, rows, K, r, T, is_put, betas8, vbar):
    """Q^_t[i] for the outer paths i in `rows`, all dates -> dict q [len(rows)][N], inner_path_steps, ties.  inner(i, t) ->
    (X, Y) of the item's inner paths, each [N - t + 1][n_inner]."""
    q = np.zeros((len(rows), N))
    steps = ties = 0
    for k, i in enumerate(rows):
        for t in range(N):
            Xi, Yi = inner(i, t)
            tau, _, Z, ti = first_stop(Xi, Yi, t, N, K, r, T, is_put, betas8, vbar)
            q[k, t] = Z.sum() / Z.size
            steps += int((tau - t).sum())
            ties += ti
    return dict(q=q, inner_path_steps=steps, ties=ties)


def walk_rows(Xo, Yo, q, rows, K, r, T, is_put, betas8, vbar):
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
            st, ti = stop_rule(x, Yo[t, i:i + 1], t, N, K, is_put, betas8, vbar)
            ties += ti
            qt = q[k, t] if t < N else 0.0
            M = M + (Zt if st[0] else qt) - q[k, t - 1]
            best = max(best, Zt - M)
        samples[k] = best
    return dict(samples=samples, ties=ties, zmax=zmax)


def upper_bound(Xo, Yo, inner, K, r, T, is_put, betas8, vbar, rows=None):
    rows = range(Xo.shape[1]) if rows is None else rows
    qr = q_rows(Xo.shape[0] - 1, inner, rows, K, r, T, is_put, betas8, vbar)
    wk = walk_rows(Xo, Yo, qr["q"], rows, K, r, T, is_put, betas8, vbar)
    up, se, ratio = br._pair_mean_se(wk["samples"]) if len(wk["samples"]) % 2 == 0 else (math.nan,) * 3
    return dict(upper=up, se_upper=se, se_cancel=ratio, q=qr["q"], samples=wk["samples"],
                inner_path_steps=qr["inner_path_steps"], ties=qr["ties"] + wk["ties"], zmax=wk["zmax"])


# ---------------------------------------------------------------------------------------------- the fit
def date_set(X, Y, t, K, r, T, is_put, betas8, vbar):
    """Date t's regression set with the later dates decided by betas8 -> (u, w, y, ties, n)"""
    N = X.shape[0] - 1
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    tau, x_ex, _, ties = first_stop(X[t:], Y[t:], t, N, K, r, T, is_put, betas8, vbar)
    xd = X[t].astype(np.float64)
    itm = (K - xd if is_put else xd - K) > 0.0
    xe = x_ex[itm].astype(np.float64)
    y = D[tau[itm] - t] * np.maximum(K - xe if is_put else xe - K, 0.0)
    u, w = uw(X[t][itm], Y[t][itm], K, vbar)
    return u, w, y, ties, int(np.count_nonzero(itm))


def fit_table(X, Y, K, r, T, is_put, vbar):
    """The textbook fit on paths (X, Y) [N+1][M], every date solved here -> (betas8, ties)"""
    N = X.shape[0] - 1
    b = np.zeros((N + 1, 8))
    ties = 0
    for t in range(N - 1, 0, -1):
        u, w, y, ti, _ = date_set(X, Y, t, K, r, T, is_put, b, vbar)
        ties += ti
        b[t] = rr.ldl_fit(u, w, y)
    return b, ties


def check_fit(X, Y, K, r, T, is_put, betas8, vbar, tol=1e-9):
    """runnerup_ref.check_fit for (spot, variance): the device's fitted table on its own fitting paths, date by date.  For
    t = N-1 .. 1 the later dates are decided with the DEVICE's rows (no ties), the row solved here; the two continuation
    values on the set agree within tol * K and n_t is equal.  -> the largest difference / K."""
    N = X.shape[0] - 1
    assert betas8.shape == (N + 1, 8) and not betas8[0].any() and not betas8[N].any()
    worst = 0.0
    for t in range(N - 1, 0, -1):
        u, w, y, ties, n = date_set(X, Y, t, K, r, T, is_put, betas8, vbar)
        assert ties == 0, (t, ties)
        row = rr.ldl_fit(u, w, y)
        assert betas8[t][6] == row[6] == n, (t, betas8[t][6], row[6], n)
        assert betas8[t][7] == 0.0
        if n > 0:
            diff = float(np.max(np.abs(rr.continuation(u, w, betas8[t]) - rr.continuation(u, w, row))))
            assert diff <= tol * K, (t, diff)
            worst = max(worst, diff / K)
        else:
            assert not betas8[t].any()
    return worst


# ---------------------------------------------------------------------------------------------- float32 Heston in numpy
def _fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def heston_consts(r, T, N, kappa, theta, xi, rho):
    dt, L2E = T / N, 1.4426950408889634074
    return dict(kdt=f32(kappa * dt), theta=f32(theta), rho=f32(rho), rho2=f32(math.sqrt(1.0 - rho * rho)),
                xi_sqdt=f32(xi * math.sqrt(dt)), l2e_sqdt=f32(L2E * math.sqrt(dt)), hdt_l2=f32(0.5 * dt * L2E),
                rdt_l2=f32(r * dt * L2E))


def paths_f32(z1, z2, s0, v0, r, T, kappa, theta, xi, rho, scheme):
    """The generator's step (schemes 0 and 1) in float32 numpy from normals z1, z2 [n][H], dt = T / n -> (S, V)
    [n+1][2 H], antithetic layout, the partner with (-z1, -z2).  V has the generator's operation order and is the
    device's but for its square root (within 1 ulp there, not correctly rounded) and what that does to a path near zero;
    S uses numpy's exp2.  Plausible paths for the checks that need no GPU, not the device's."""
    n, H = z1.shape
    c = heston_consts(r, T, n, kappa, theta, xi, rho)
    S, V = np.zeros((n + 1, 2 * H), f32), np.zeros((n + 1, 2 * H), f32)
    S[0], V[0] = f32(s0), f32(v0)
    for k in range(n):
        a, b = z1[k].astype(f32), z2[k].astype(f32)
        w2 = _fma32(np.full(H, c["rho"]), a, c["rho2"] * b)
        tw, az = c["xi_sqdt"] * w2, c["l2e_sqdt"] * a
        tw, az = np.concatenate([tw, -tw]), np.concatenate([az, -az])
        v = V[k]
        vp = np.maximum(v, f32(0.0))
        sq = np.sqrt(vp)
        kd, th = np.full(2 * H, c["kdt"]), np.full(2 * H, c["theta"])
        vn = _fma32(sq, tw, _fma32(kd, th - vp, v if scheme else vp))
        arg = _fma32(sq, az, _fma32(np.full(2 * H, -c["hdt_l2"]), vp, np.full(2 * H, c["rdt_l2"])))
        S[k + 1] = S[k] * np.exp2(arg)
        V[k + 1] = vn if scheme else np.maximum(vn, f32(0.0))
    return S, V


# ---------------------------------------------------------------------------------------------- the device's own states
def paths_sv(ctx, p, n_paths, stream, pair_offset=0, S0=None, v0=None):
    hp = hc.hp_of(p)
    if v0 is not None:
        hp = [v0] + hp[1:]
    Sd, Vd = ctx.heston_paths_sv(n_paths, int(p.n_steps), p.S0 if S0 is None else S0, p.r, p.T, *hp, p.seed, stream,
                                 pair_offset, int(p.heston_scheme))
    return hc.host(Sd), hc.host(Vd)


def fitting_paths(ctx, p):
    return paths_sv(ctx, p, int(p.n_paths), p.stream, p.pair_offset)


def device_states(ctx, p, n_lower, n_outer, n_inner, streams=None, cache=False):
    """-> dict Xl, Yl (lower paths), Xo, Yo (outer paths) and inner(i, t) -> (X, Y) [N - t + 1][n_inner]; cache=True computes
    every item once (for cases that several tests share)."""
    N = int(p.n_steps)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Xl, Yl = paths_sv(ctx, p, n_lower, s_lo)
    Xo, Yo = paths_sv(ctx, p, n_outer, s_out)
    H = n_inner // 2

    def inner(i, t):
        S, V = paths_sv(ctx, p, n_inner, s_in, (i * (N + 1) + t) * H, float(Xo[t, i]), float(Yo[t, i]))
        return S[:N - t + 1], V[:N - t + 1]

    if cache:
        items = {(i, t): inner(i, t) for i in range(n_outer) for t in range(N)}
        return dict(Xl=Xl, Yl=Yl, Xo=Xo, Yo=Yo, inner=lambda i, t: items[(i, t)])
    return dict(Xl=Xl, Yl=Yl, Xo=Xo, Yo=Yo, inner=inner)


def check_against_restatement(p, dev, st, n_lower, n_outer, n_inner, rtol=1e-12):
    """heston_bounds_case.check_against_restatement for the two-regressor policy dev["betas"] [N+1][8] on the device's own
    states `st` (device_states)"""
    K, is_put, vb = float(p.K), bool(p.is_put), vbar_of(p)
    lo = lower_bound(st["Xl"], st["Yl"], K, p.r, p.T, is_put, dev["betas"], vb)
    up = upper_bound(st["Xo"], st["Yo"], st["inner"], K, p.r, p.T, is_put, dev["betas"], vb)
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


def given_table(ctx, p, holes=None):
    """a two-regressor policy from other paths (2048 of stream 9 of p's seed), with n = 0 on the dates `holes` marks"""
    q = type(p).from_buffer_copy(bytes(p))
    q.n_paths, q.stream, q.pair_offset = 2048, 9, 0
    d = ctx.price_american_bounds_heston(q, policy="textbook", n_lower=2, n_outer=2, n_inner=2, regressors=REG)
    t = d["betas"].copy()
    if holes is not None:
        t[np.asarray(holes), 6] = 0.0
    return t


def spot_table(betas8):
    """(c0, c1, c2, n) of a table whose c3 = c4 = c5 = 0: the spot-only call's [N+1][4]"""
    assert not betas8[:, 3:6].any()
    return np.ascontiguousarray(betas8[:, [0, 1, 2, 6]])


def lifted_table(betas4):
    """the [N+1][8] table that decides as the spot-only betas4 = (b0, b1, b2, n)"""
    t = np.zeros((betas4.shape[0], 8))
    t[:, :3], t[:, 6] = betas4[:, :3], betas4[:, 3]
    return t


# ---------------------------------------------------------------------------------------------- the fuzz cases
def fuzz_cases(n, seed=20261021):
    """n seeded cases of the fuzz sweep: heston_bounds_case.fuzz_cases' shapes and laws (N in 1 .. 13, n_inner of its
    N_INNER, a ragged even n_outer, schemes 0 and 1, put / call, every third case violating Feller) with the policies of
    this family: fitted (textbook) on the even cases, a given table with n = 0 holes on the odd ones."""
    out = hc.fuzz_cases(n, seed)
    for k, c in enumerate(out):
        c["policy"] = POLICIES[k % 2]
        del c["irr_every"]  # no exercise tables here
    return out

"""numpy restatement of the running-average (Asian) index kinds (OMC_BASKET_ASIAN_ARITHMETIC / _GEOMETRIC; the definitions
are in include/omc.h and DESIGN.md section 23).  TEST INFRASTRUCTURE ONLY.

  basket_value      B_t of asset matrices by the float32 rule of OMC_BASKET_ARITHMETIC: wf_0 s_0, then fmaf(wf_k, s_k, B)
                    with k ascending.  numpy has no float32 fma; fmaf32 forms the exact product in float64 (48 bits), adds
                    with the error of the sum known (two-sum) and rounds to odd before the float32 rounding: exactly fmaf.
  arithmetic_index  the arithmetic kind bit for bit: c_t = c_{t-1} + B_t (float32), X_t = c_t * (1.0f / (float)t), X_0 = B_0
  geometric_index   the geometric kind in float64: X_t = exp2(sum log2 B_s / t); the device uses the hardware log2 / exp2 in float32
  geometric_asian_european   the discrete geometric-average closed form of one GBM asset with a yield
and, for the bounds, the device's own spots as helpers/basket_bounds_case.py builds them: lower and outer paths from
omc_price_american_basket at kind "asian", the inner paths of item (i, t) from a RESTART call of kind "basket" at the outer asset
spots A_k[t][i] -- rows of asset spots, which carry no state -- continued here from the rebuilt outer state c_t[i].
The two-regressor rule, estimators and fit are helpers/runnerup_ref.py's with (X, Y) = (average, basket value).
"""
from __future__ import annotations

import math

import numpy as np

from helpers import basket_bounds_case as bc
from helpers import bounds_ref as br
from helpers import runnerup_ref as rr
from options_model_amd import _ffi

REG = "index+spot"
KINDS = ("asian", "asian-geometric")


# ---------------------------------------------------------------------------------------------- the index rules
def fmaf32(a, b, c):
    """float32 fma(a, b, c), exactly: round32(a b + c) with one rounding"""
    a64, b64, c64 = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a64 * b64  # exact: 24 + 24 bits
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)  # two-sum: p + c = s + err exactly
    bits = np.atleast_1d(s).view(np.int64)
    fix = (np.atleast_1d(err) != 0.0) & ((bits & 1) == 0) & np.isfinite(np.atleast_1d(s))
    toward = np.where(np.atleast_1d(err) > 0.0, np.inf, -np.inf)
    odd = np.where(fix, np.nextafter(np.atleast_1d(s), toward), np.atleast_1d(s))  # round to odd: the sticky bit
    return odd.reshape(np.shape(s)).astype(np.float32)


def basket_value(A, w):
    """A [d][...] float32 asset spots, w [d] -> B [...] float32 by the rule of OMC_BASKET_ARITHMETIC"""
    A = np.asarray(A, np.float32)
    wf = np.asarray(w, np.float64).astype(np.float32)
    B = wf[0] * A[0]
    for k in range(1, A.shape[0]):
        B = fmaf32(np.broadcast_to(wf[k], A[k].shape), A[k], B)
    return B.astype(np.float32)


def continue_arithmetic(B, c0, t0):
    """B [n][m] float32: the basket values of dates t0 + 1 .. t0 + n of paths whose running sum at t0 is c0 (scalar or
    [m]) -> (X [n][m], c [n][m]) float32 by the arithmetic rule"""
    B = np.asarray(B, np.float32)
    c = np.broadcast_to(np.asarray(c0, np.float32), B.shape[1:]).copy()
    X, C = np.empty_like(B), np.empty_like(B)
    for k in range(B.shape[0]):
        c = (c + B[k]).astype(np.float32)
        inv = np.float32(1.0) / np.float32(t0 + k + 1)
        X[k], C[k] = (c * inv).astype(np.float32), c
    return X, C


def arithmetic_index(A, w):
    """A [d][N+1][M] float32 -> (X, B, c) [N+1][M] float32: the arithmetic index matrix, the basket values, the running sums
    (c_0 = 0, X_0 = B_0)"""
    B = basket_value(A, w)
    X, c = np.empty_like(B), np.zeros_like(B)
    X[0] = B[0]
    if B.shape[0] > 1:
        X[1:], c[1:] = continue_arithmetic(B[1:], np.float32(0.0), 0)
    return X, B, c


def geometric_index(A, w):
    """A [d][N+1][M] float32 -> X [N+1][M] float64 of the geometric kind: exp2(mean of log2 B_1 .. B_t), X_0 = B_0"""
    B = basket_value(A, w).astype(np.float64)
    X = np.empty_like(B)
    X[0] = B[0]
    t = np.arange(1, B.shape[0])[:, None]
    X[1:] = np.exp2(np.cumsum(np.log2(B[1:]), axis=0) / t)
    return X


# ---------------------------------------------------------------------------------------------- the closed form
def geometric_moments(S0, r, q, sigma, T, N):
    """ln G of the geometric average of S at the grid dates 1 .. N (dt = T / N) ~ N(mean, var)"""
    dt = T / N
    mean = math.log(S0) + (r - q - 0.5 * sigma * sigma) * dt * (N + 1) / 2.0
    var = sigma * sigma * dt * (N + 1) * (2 * N + 1) / (6.0 * N)
    return mean, var


def geometric_asian_european(S0, K, r, q, sigma, T, N, is_put):
    """exp(-r T) E max(K - G, 0) / max(G - K, 0) for the lognormal G of geometric_moments"""
    m, v = geometric_moments(S0, r, q, sigma, T, N)
    sd = math.sqrt(v)
    d1 = (m - math.log(K) + v) / sd
    d2 = d1 - sd
    fwd = math.exp(m + 0.5 * v)
    if is_put:
        return math.exp(-r * T) * (K * br._ncdf(-d2) - fwd * br._ncdf(-d1))
    return math.exp(-r * T) * (fwd * br._ncdf(d1) - K * br._ncdf(d2))


def gbm_paths64(rng, n, S0, r, q, sigma, T, N):
    """plain float64 paths [N][n] of one GBM asset at the grid dates 1 .. N"""
    dt = T / N
    z = rng.standard_normal((N, n))
    return S0 * np.exp(np.cumsum((r - q - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * z, axis=0))


# ---------------------------------------------------------------------------------------------- the device's own spots
def weights(b):
    return [float(b.w[k]) for k in range(int(b.n_assets))]


def as_kind(b, kind):
    return bc.with_fields(b, kind=_ffi.BASKET_KINDS[kind])


def paths(ctx, p, b):
    """(S, A, X, B, c) of omc_price_american_basket(p, b) at kind "asian": the device's index and assets, the restatement"""
    S, A = bc.index_and_assets(ctx, p, b)
    return (S, A) + arithmetic_index(A, weights(b))


def device_spots(ctx, p, b, n_lower, n_outer, n_inner, streams=None):
    """b of kind "asian" -> dict Xl, Bl (lower paths), Xo, Bo, Co (outer paths: index, basket value, running sum), Ao and
    inner(i, t) -> (X, B) [N - t + 1][n_inner] with row 0 = (Xo[t][i], Bo[t][i]).  The lower and outer index matrices are
    the device's, asserted equal to the restatement bit for bit."""
    N, d = int(p.n_steps), int(b.n_assets)
    w = weights(b)
    s_lo, s_out, s_in = streams or (p.stream + 1, p.stream + 2, p.stream + 3)
    Sl, _, Xl, Bl, _ = paths(ctx, bc.with_fields(p, n_paths=n_lower, stream=s_lo, pair_offset=0), b)
    So, Ao, Xo, Bo, Co = paths(ctx, bc.with_fields(p, n_paths=n_outer, stream=s_out, pair_offset=0), b)
    np.testing.assert_array_equal(Sl.view(np.uint32), Xl.view(np.uint32))
    np.testing.assert_array_equal(So.view(np.uint32), Xo.view(np.uint32))
    H = n_inner // 2
    plain = as_kind(b, "basket")
    keep = ctx.empty((N + 1, n_inner), np.float32)
    akeep = ctx.empty((d, N + 1, n_inner), np.float32)

    def inner(i, t):
        rb = bc.with_fields(plain)
        for k in range(d):
            rb.S0[k] = float(Ao[k, t, i])
        ctx.price_american_basket(bc.with_fields(p, n_paths=n_inner, stream=s_in, pair_offset=(i * (N + 1) + t) * H), rb,
                                  S_keep=keep, assets_keep=akeep)
        B = basket_value(akeep.to_host()[:, :N - t + 1], w)
        X = np.empty_like(B)
        X[0] = Xo[t, i]
        if N > t:
            X[1:], _ = continue_arithmetic(B[1:], Co[t, i], t)
        return X, B

    def free():
        keep.free()
        akeep.free()

    return dict(Xl=Xl, Bl=Bl, Xo=Xo, Bo=Bo, Co=Co, Ao=Ao, inner=inner, free=free)


def _compare(p, dev, lo, up, n_lower, n_outer, n_inner, rtol):
    K = float(p.K)
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


def check_against_restatement(ctx, p, b, dev, n_lower, n_outer, n_inner, regressors="index", rtol=1e-12, sp=None):
    """The device's result dict `dev` (want_q, want_samples) of kind "asian" against the restatement on the device's own
    spots: no ties, equal counts, q / samples / bounds at rtol (atol rtol K).  regressors "index": dev["betas"] [N+1][4]
    and bounds_ref; "index+spot": [N+1][8] and runnerup_ref with (X, Y) = (average, basket value)."""
    K, is_put = float(p.K), bool(p.is_put)
    own = sp is None
    sp = sp or device_spots(ctx, p, b, n_lower, n_outer, n_inner)
    try:
        if regressors == "index":
            lo = br.lower_bound(sp["Xl"], K, p.r, p.T, is_put, dev["betas"])
            up = br.upper_bound(sp["Xo"], lambda i, t: sp["inner"](i, t)[0], K, p.r, p.T, is_put, dev["betas"])
        else:
            lo = rr.lower_bound(sp["Xl"], sp["Bl"], K, p.r, p.T, is_put, dev["betas"])
            up = rr.upper_bound(sp["Xo"], sp["Bo"], sp["inner"], K, p.r, p.T, is_put, dev["betas"])
    finally:
        if own:
            sp["free"]()
    _compare(p, dev, lo, up, n_lower, n_outer, n_inner, rtol)
    return lo, up


def given_table4(ctx, p, b, holes=None):
    """an index policy from other paths (2048 of stream 9 of p's seed), textbook fits on the kind's own index matrix"""
    t = bc.fitted_table(ctx, bc.with_fields(p, n_paths=2048, stream=9, pair_offset=0), b, "textbook")
    if holes is not None:
        t[np.asarray(holes), 3] = 0.0
    return t


def given_table8(ctx, p, b, holes=None):
    """a two-regressor policy from other paths (2048 of stream 9 of p's seed), with n = 0 on the dates `holes` marks"""
    d = ctx.price_american_basket_bounds(bc.with_fields(p, n_paths=2048, stream=9, pair_offset=0), b, policy="textbook",
                                         n_lower=2, n_outer=2, n_inner=2, regressors=REG)
    t = d["betas"].copy()
    if holes is not None:
        t[np.asarray(holes), 6] = 0.0
    return t


# ---------------------------------------------------------------------------------------------- the fuzz cases
N_INNER = (2, 64, 130, 200)


def fuzz_cases(n, seed=20261019):
    """n seeded cases of the fuzz sweep, as plain dicts: kind "asian" with d in 1 .. 8 (a permutation, cycled), N in 1 .. 13,
    n_inner of N_INNER (at least a third with more inner pairs than a wave has lanes: the refill), a ragged n_outer, put /
    call, the regressors alternating, the policy fitted or (every third case) given with n = 0 holes."""
    rng = np.random.default_rng(seed)
    perm_d = rng.permutation(8)
    out = []
    for c in range(n):
        d = int(perm_d[c % 8]) + 1
        n_inner = N_INNER[3 - c % 4] if c % 3 else int(rng.choice((130, 200)))
        N = int(rng.integers(1, 14))
        case = dict(d=d, kind="asian", N=N, n_inner=n_inner, n_outer=2 * int(rng.integers(1, 12)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy="given" if c % 3 == 2 else "textbook",
                    regressors=("index", REG)[c % 2], seed=int(rng.integers(1, 1 << 31)), stream=int(rng.integers(0, 50)),
                    S0=[float(x) for x in rng.uniform(85.0, 115.0, d)], sigma=[float(x) for x in rng.uniform(0.1, 0.4, d)],
                    q=[float(x) for x in rng.uniform(0.0, 0.08, d)], rho=bc.random_correlation(rng, d),
                    T=float(rng.uniform(0.5, 3.0)))
        w = rng.uniform(0.5, 1.5, d)
        case["w"] = [float(x) for x in w / w.sum()]
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]  # dates of a given table with n = 0
        case["refill"] = n_inner // 2 > 64
        out.append(case)
    return out

"""numpy restatement of the GBM price bounds with the Black-Scholes control variate (option "bounds_control_variate" = 1;
the definitions are in DESIGN.md section 26 and include/omc.h), built on tests/helpers/bounds_ref.py and
bounds_schedule_ref.py.  TEST INFRASTRUCTURE ONLY.

dt = T / N, D[t] = exp(-r dt t), x = float64 of a float32 spot.  E(x, d) is the Black-Scholes value (no dividend yield) of
the European put / call at spot x, strike K and time to expiry (N - d) dt, float64 with Phi(y) = erfc(-y / sqrt 2) / 2.
The discounted European value D_t E(S_t, t) is a martingale on the grid, so for a stopping time tau > t
    control = D[tau] E(S_tau, tau)   (tau < N),      control = Z   (tau = N: E at expiry is the payoff)
has conditional mean D[t] E(S_t, t), and a stopped partner contributes c = Z - control: exactly 0.0 at tau = N.
Paths, stopping rule, policy and walk are those of the plain bounds; only what is averaged changes:
    Q^_t[i] = D[t] E(S_t[i], t) + mean(c over the item's inner paths)
    lower   = E0 + mean of the pair means (c_a + c_b) / 2,  E0 = D[0] E(float32(S0), 0);  se_lower from those pair means
"""
from __future__ import annotations

import math

import numpy as np

from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs

# The worst deviations of the device from this restatement over the restated, lane-group, never-exercising, two-launch and fuzz
# cases of tests/test_gpu_bounds_cv.py and test_gpu_bounds_cv_fuzz.py, in units of K, and the tests' bounds: 4 times them.
#   q 3.553e-16, lower 7.105e-17                    -> MEASURED, CV_TOL: Q^ and the lower bound
#   samples 5.329e-16, upper 8.882e-17              -> MEASURED_WALK, CV_TOL_WALK: what has been through the walk
MEASURED = 3.6e-16
CV_TOL = 4 * MEASURED
MEASURED_WALK = 5.4e-16
CV_TOL_WALK = 4 * MEASURED_WALK

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def phi(y):
    return 0.5 * _erfc(-np.asarray(y, np.float64) / math.sqrt(2.0))


def euro(x, d, N, K, r, sigma, T, is_put):
    """E(x, d) for spots x (any shape, read as float64) at date(s) d < N (scalar or of x's shape)"""
    x = np.asarray(x, np.float64)
    tau = (N - np.asarray(d, np.float64)) * (T / N)
    sq = sigma * np.sqrt(tau)
    d1 = (np.log(x / K) + (r + 0.5 * sigma * sigma) * tau) / sq
    d2 = d1 - sq
    sg = -1.0 if is_put else 1.0
    return sg * (x * phi(sg * d1) - K * np.exp(-r * tau) * phi(sg * d2))


def discounts(N, r, T):
    return np.exp(-r * (T / N) * np.arange(N + 1))


def e0(S0, N, K, r, sigma, T, is_put):
    """E0 = D[0] E((double)(float)S0, 0)"""
    return float(euro(np.float64(np.float32(S0)), 0, N, K, r, sigma, T, is_put))


def stopped(S, t0, N, K, r, T, is_put, betas4):
    """bounds_ref.first_stop with the spot each path stopped at -> (tau, x float32, Z, ties)"""
    tau, Z, ties = br.first_stop(S, t0, N, K, r, T, is_put, betas4)
    x = S[tau - t0, np.arange(S.shape[1])]
    return tau, x, Z, ties


def control(tau, x, Z, N, K, r, sigma, T, is_put):
    """D[tau] E(S_tau, tau) where tau < N, Z itself where tau = N (nothing evaluated there)"""
    D = discounts(N, r, T)
    out = np.array(Z, np.float64)
    early = tau < N
    if np.any(early):
        out[early] = D[tau[early]] * euro(x[early], tau[early], N, K, r, sigma, T, is_put)
    return out


def terms(tau, x, Z, N, K, r, sigma, T, is_put):
    """c = Z - control: exactly 0.0 at tau = N"""
    c = Z - control(tau, x, Z, N, K, r, sigma, T, is_put)
    c[tau >= N] = 0.0
    return c


def lower_bound(S, K, r, sigma, T, is_put, betas4, k=0):
    """S: the lower-bound paths [N+1][n_lower] (antithetic layout) -> dict lower, se_lower, n_exercised, ties, e0, c"""
    N = S.shape[0] - 1
    tau, x, Z, ties = stopped(S, 0, N, K, r, T, is_put, bs.mask(betas4, k))
    c = terms(tau, x, Z, N, K, r, sigma, T, is_put)
    mean, se, ratio = br._pair_mean_se(c)
    E0 = float(euro(S[0, 0], 0, N, K, r, sigma, T, is_put))
    return dict(lower=E0 + mean, se_lower=se, se_cancel=ratio, n_exercised=int(np.count_nonzero(tau < N)), ties=ties, e0=E0,
                c=c, Z=Z)


def q_rows(So, inner, rows, K, r, sigma, T, is_put, betas4, k=0):
    """The controlled Q^ of the outer paths in `rows` at the dates of the schedule k (0: every date) -> dict q [len(rows)][N]
    (zero off those columns), q_plain (the plain means on the same inner paths), inner_path_steps, ties."""
    N = So.shape[0] - 1
    D = discounts(N, r, T)
    bk = bs.mask(betas4, k)
    q = np.zeros((len(rows), N))
    qp = np.zeros((len(rows), N))
    steps = ties = 0
    for m, i in enumerate(rows):
        for t in bs.schedule(N, k)[:-1]:
            tau, x, Z, ti = stopped(inner(i, t), t, N, K, r, T, is_put, bk)
            c = terms(tau, x, Z, N, K, r, sigma, T, is_put)
            q[m, t] = D[t] * float(euro(So[t, i], t, N, K, r, sigma, T, is_put)) + math.fsum(c) / c.size
            qp[m, t] = Z.sum() / Z.size
            steps += int((tau - t).sum())
            ties += ti
    return dict(q=q, q_plain=qp, inner_path_steps=steps, ties=ties)


def upper_bound(So, inner, K, r, sigma, T, is_put, betas4, k=0):
    rows = range(So.shape[1])
    qr = q_rows(So, inner, rows, K, r, sigma, T, is_put, betas4, k)
    wk = bs.walk_rows(So, qr["q"], rows, K, r, T, is_put, betas4, k)
    up, se, ratio = br._pair_mean_se(wk["samples"])
    return dict(upper=up, se_upper=se, se_cancel=ratio, q=qr["q"], q_plain=qr["q_plain"], samples=wk["samples"],
                inner_path_steps=qr["inner_path_steps"], ties=qr["ties"] + wk["ties"], zmax=wk["zmax"])


def never_exercising(So, K, r, sigma, T, is_put, k=0):
    """What a table that never exercises gives, with no inner path: q[i][t] = D[t] E(S_t[i], t) at the scheduled t < N, and
    samples[i] = Q_0 + max(0, max over the scheduled 1 <= t < N of Z_t - q[i][t]) -> dict q, samples"""
    N, n = So.shape[0] - 1, So.shape[1]
    D = discounts(N, r, T)
    ts = bs.schedule(N, k)[:-1]
    q = np.zeros((n, N))
    for t in ts:
        q[:, t] = D[t] * euro(So[t], t, N, K, r, sigma, T, is_put)
    best = np.zeros(n)
    for t in ts[1:]:
        phi_ = (K - So[t].astype(np.float64)) if is_put else (So[t].astype(np.float64) - K)
        best = np.maximum(best, D[t] * np.maximum(phi_, 0.0) - q[:, t])
    return dict(q=q, samples=q[:, 0] + best)


def deviations(dev, lo, up, K):
    """the largest deviations of a device result (want_q, want_samples) from the restatement, in units of K"""
    return dict(q=float(np.max(np.abs(dev["q"] - up["q"]), initial=0.0)) / K,
                samples=float(np.max(np.abs(dev["samples"] - up["samples"]), initial=0.0)) / K,
                lower=abs(dev["lower"] - lo["lower"]) / K, se_lower=abs(dev["se_lower"] - lo["se_lower"]) / K,
                upper=abs(dev["upper"] - up["upper"]) / K, se_upper=abs(dev["se_upper"] - up["se_upper"]) / K)


def se_atol(se, ratio, mean, P, delta=16 * 2.0 ** -53):
    """What the device's standard error sqrt((E[m^2] - mean^2) / P) may differ by from the exactly rounded one of
    bounds_ref._pair_mean_se, whatever the samples: its two float64 sums and the subtraction leave an error of at most
    delta E[m^2] in the variance (a handful of roundings), and |sqrt(a + e) - sqrt(a)| <= min(sqrt |e|, |e| / sqrt a).  With
    ratio = E[m^2] / Var[m]; zero variance: E[m^2] = mean^2."""
    e2 = ratio * se * se * P if se > 0.0 else mean * mean
    loose = math.sqrt(delta * e2 / P)
    return loose if se <= loose else min(loose, delta * e2 / (se * P))


def check_against_restatement(p, dev, sp, k, n_lower, n_outer, n_inner, tol=CV_TOL, tol_walk=CV_TOL_WALK):
    """The device's dict `dev` of a controlled call (want_q, want_samples) against the restatement on the device's own spots
    `sp` (Sl, So, inner): no ties, equal counts, q and lower within tol K, samples and upper within tol_walk K -- each 4 times
    its own measured worst.  The standard errors get se_atol, the cancellation of the device's own formula, beside that.
    -> the deviations in units of K"""
    K, is_put = float(p.K), bool(p.is_put)
    lo = lower_bound(sp["Sl"], K, p.r, p.sigma, p.T, is_put, dev["betas"], k)
    up = upper_bound(sp["So"], sp["inner"], K, p.r, p.sigma, p.T, is_put, dev["betas"], k)
    assert lo["ties"] == 0 and up["ties"] == 0  # numpy's decisions are the device's
    assert dev["n_exercised_lower"] == lo["n_exercised"]
    assert dev["inner_path_steps"] == up["inner_path_steps"]
    dv = deviations(dev, lo, up, K)
    assert dv["q"] <= tol and dv["lower"] <= tol, dv
    assert dv["samples"] <= tol_walk and dv["upper"] <= tol_walk, dv
    assert dv["se_lower"] * K <= tol * K + se_atol(lo["se_lower"], lo["se_cancel"], lo["lower"] - lo["e0"], n_lower // 2), dv
    assert dv["se_upper"] * K <= tol_walk * K + se_atol(up["se_upper"], up["se_cancel"], up["upper"], n_outer // 2), dv
    assert dev["ci_lo"] == dev["lower"] - 1.96 * dev["se_lower"] and dev["ci_hi"] == dev["upper"] + 1.96 * dev["se_upper"]
    assert (dev["n_lower"], dev["n_outer"], dev["n_inner"]) == (n_lower, n_outer, n_inner)
    return dv


# ---------------------------------------------------------------------------------------------- the fuzz cases
def fuzz_cases(n, seed=20261021):
    """n seeded GBM cases, as plain dicts: N in 1 .. 13, every third with a schedule k in 2 .. N + 3, n_inner over every lane
    group, a ragged group and the refill, a ragged even n_outer, put / call, fitted policies and given tables with n = 0
    holes, the float64 fallback on some"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        N = int(rng.integers(1, 14))
        case = dict(N=N, k=int(rng.integers(2, N + 4)) if c % 3 == 2 else 0, model="gbm",
                    n_inner=(2, 16, 24, 64, 66, 192, 10, 130)[c % 8], n_outer=2 * int(rng.integers(1, 21)),
                    n_lower=2 * int(rng.integers(100, 700)), M=2 * int(rng.integers(300, 1500)),
                    is_put=bool(rng.integers(0, 2)), policy=("textbook", "given", "two_pass", "reference")[(c + c // 4) % 4],
                    irr_every=int(rng.choice((0, 0, 1, 2, 3))), seed=int(rng.integers(1, 1 << 31)),
                    stream=int(rng.integers(0, 50)), S0=100.0 * float(rng.uniform(0.8, 1.25)), K=100.0,
                    r=float(rng.uniform(0.0, 0.08)), T=float(rng.uniform(0.5, 3.0)), sigma=float(rng.uniform(0.1, 0.5)))
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]
        out.append(case)
    return out

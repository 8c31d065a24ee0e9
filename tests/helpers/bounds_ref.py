"""numpy restatement of the Andersen-Broadie price bounds (omc_price_american_bounds; the definitions are in DESIGN.md
section 12 and include/omc.h) and the Bermudan value of the game by backward induction.  TEST INFRASTRUCTURE ONLY.

The game: exercise dates t = 1..N on dt = T / N, Z_t = exp(-r t dt) max(phi(S_t), 0).  The policy betas4 [N+1][4] =
b0, b1, b2, n: at 1 <= t < N a path at spot s exercises iff n > 0.5, imm = phi(s) > 0 and imm > b0 + b1 u + b2 u^2
(u = s / K - 1); at N it takes its payoff.  Decisions, discounting and sums are numpy float64; the spots are the caller's
(the device's own generators, or the C oracle's).  numpy has no fused multiply-add, so a decision within TIE * K of the
continuation value is counted as a tie: where there are none, the decisions are the device's.
"""
from __future__ import annotations

import math

import numpy as np

TIE = 1e-10


def _ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def black_scholes(S0, K, r, sigma, T, is_put=True):
    d1 = (math.log(S0 / K) + (r + 0.5 * sigma * sigma) * T) / (sigma * math.sqrt(T))
    d2 = d1 - sigma * math.sqrt(T)
    if is_put:
        return K * math.exp(-r * T) * _ncdf(-d2) - S0 * _ncdf(-d1)
    return S0 * _ncdf(d1) - K * math.exp(-r * T) * _ncdf(d2)


# ---------------------------------------------------------------------------------------------- Bermudan lattice
def lattice(S0, K, r, sigma, T, N, is_put=True, n_sd=7.0, h=1e-3):
    """Value of the game by backward induction on a uniform log-spot grid through S0 (and K) with Gaussian transition
    weights: the value function is interpolated linearly in x = log S between nodes and the expectation of that
    interpolant under the one-step law N(x + (r - sigma^2/2) dt, sigma^2 dt) is exact (hat functions against the normal
    law; constant beyond the grid).  The last step uses the exact one-period European value."""
    dt = T / N
    mu, s = (r - 0.5 * sigma * sigma) * dt, sigma * math.sqrt(dt)
    x0 = math.log(S0)
    if S0 != K:  # K on a node too: the payoff's kink then costs no interpolation error
        span = abs(math.log(K / S0))
        h = span / max(1, round(span / h))
    half = int(math.ceil(n_sd * sigma * math.sqrt(T) / h)) + 2
    x = x0 + h * np.arange(-half, half + 1)
    n = x.size
    S = np.exp(x)
    pay = np.maximum(K - S, 0.0) if is_put else np.maximum(S - K, 0.0)
    disc = math.exp(-r * dt)

    def G(m):  # E[(X - a)^+], X ~ N(a + m, s^2)
        d = m / s
        return m * _ncdf(d) + s * math.exp(-0.5 * d * d) / math.sqrt(2.0 * math.pi)

    g = np.array([G(k * h + mu) for k in range(-n - 1, n + 2)])  # g[k + n + 1] = G(k h + mu), k = j - i offsets
    gi = lambda k: g[k + n + 1]  # noqa: E731
    j = np.arange(n)[:, None]
    i = np.arange(n)[None, :]
    W = (gi(j - i + 1) - 2.0 * gi(j - i) + gi(j - i - 1)) / h  # source node j, target hat i
    jj = np.arange(n)
    W[:, 0] = 1.0 - (gi(jj) - gi(jj - 1)) / h  # left hat held constant below the grid
    W[:, n - 1] = (gi(jj - n + 2) - gi(jj - n + 1)) / h  # right hat held constant above it

    def euro1(Sv):  # exact E[disc max(phi(S_N), 0) | S_{N-1} = Sv]
        return np.array([black_scholes(v, K, r, sigma, dt, is_put) for v in Sv])

    if N == 1:
        return float(euro1([S0])[0])
    V = np.maximum(pay, euro1(S))  # t = N - 1
    for _ in range(N - 2, 0, -1):
        V = np.maximum(pay, disc * (W @ V))
    return float(disc * (W @ V)[half])


# ---------------------------------------------------------------------------------------------- the two estimators
def stop_rule(s, t, N, K, is_put, betas4):
    """-> (stops [bool], ties [int]) for float32 spots s at date t."""
    if t >= N:
        return np.ones(s.shape, bool), 0
    b0, b1, b2, n = betas4[t]
    if not n > 0.5:
        return np.zeros(s.shape, bool), 0
    sd = s.astype(np.float64)
    imm = K - sd if is_put else sd - K
    u = sd * (1.0 / K) - 1.0
    cont = u * (u * b2 + b1) + b0
    itm = imm > 0.0
    return itm & (imm > cont), int(np.count_nonzero(itm & (np.abs(imm - cont) <= TIE * K)))


def first_stop(S, t0, N, K, r, T, is_put, betas4):
    """Paths S [N - t0 + 1][m] (row k = date t0 + k): tau = first date > t0 where the rule fires -> (tau, Z, ties)."""
    m = S.shape[1]
    tau = np.full(m, -1, np.int64)
    x = np.zeros(m, np.float32)
    ties = 0
    for k in range(1, N - t0 + 1):
        st, ti = stop_rule(S[k], t0 + k, N, K, is_put, betas4)
        live = tau < 0
        ties += ti if k + t0 < N else 0
        ex = live & st
        tau[ex] = t0 + k
        x[ex] = S[k][ex]
    phi = (K - x.astype(np.float64)) if is_put else (x.astype(np.float64) - K)
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    return tau, D[tau] * np.maximum(phi, 0.0), ties


def _pair_mean_se(x):
    """Pair means m of an antithetic layout -> (mean, standard error, E[m^2] / Var[m]).  Both sums are math.fsum: exactly
    rounded, so against a device sum only the device's own rounding counts.  The ratio is what the subtraction
    E[m^2] - mean^2 loses to cancellation (1.0 where the variance is zero)."""
    P = x.size // 2
    m = 0.5 * (x[:P] + x[P:])
    mean = math.fsum(m) / P
    e2 = math.fsum(m * m) / P
    var = max(e2 - mean * mean, 0.0)
    return mean, math.sqrt(var / P), (e2 / var if var > 0.0 else 1.0)


def lower_bound(S, K, r, T, is_put, betas4):
    """S: the n_lower lower-bound paths [N+1][n_lower] (antithetic layout) -> dict lower, se_lower, se_cancel (E[m^2] /
    Var[m] of the pair means), n_exercised, ties."""
    N = S.shape[0] - 1
    tau, Z, ties = first_stop(S, 0, N, K, r, T, is_put, betas4)
    lo, se, ratio = _pair_mean_se(Z)
    return dict(lower=lo, se_lower=se, se_cancel=ratio, n_exercised=int(np.count_nonzero(tau < N)), ties=ties)


def q_rows(So, inner, rows, K, r, T, is_put, betas4):
    """Q^_t[i] for the outer paths i in `rows`, all dates t = 0..N-1 -> dict q [len(rows)][N], inner_path_steps, ties."""
    N = So.shape[0] - 1
    q = np.zeros((len(rows), N))
    steps = 0
    ties = 0
    for k, i in enumerate(rows):
        for t in range(N):
            tau, Z, ti = first_stop(inner(i, t), t, N, K, r, T, is_put, betas4)
            q[k, t] = Z.sum() / Z.size
            steps += int((tau - t).sum())
            ties += ti
    return dict(q=q, inner_path_steps=steps, ties=ties)


def walk_rows(So, q, rows, K, r, T, is_put, betas4):
    """The martingale walk of the outer paths i in `rows` with their Q^ q [len(rows)][N] -> dict samples [len(rows)]
    (max_t Z_t - M^_t), ties, zmax (the largest Z_t met: the scale of the walk's rounding)."""
    N = So.shape[0] - 1
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    samples = np.zeros(len(rows))
    ties = 0
    zmax = 0.0
    for k, i in enumerate(rows):
        M, best = 0.0, -math.inf
        for t in range(1, N + 1):
            s = So[t, i:i + 1]
            phi = (K - float(s[0])) if is_put else (float(s[0]) - K)
            Zt = D[t] * max(phi, 0.0)
            zmax = max(zmax, Zt)
            st, ti = stop_rule(s, t, N, K, is_put, betas4)
            ties += ti
            qt = q[k, t] if t < N else 0.0
            L = Zt if st[0] else qt
            M = M + L - q[k, t - 1]
            best = max(best, Zt - M)
        samples[k] = best
    return dict(samples=samples, ties=ties, zmax=zmax)


def upper_bound(So, inner, K, r, T, is_put, betas4):
    """So: outer paths [N+1][n_outer]; inner(i, t) -> the inner paths of item (i, t) as [N - t + 1][n_inner] float32 (row
    0 = S_t[i]).  -> dict upper, se_upper, se_cancel, q [n_outer][N], samples [n_outer], inner_path_steps, ties, zmax."""
    rows = range(So.shape[1])
    qr = q_rows(So, inner, rows, K, r, T, is_put, betas4)
    wk = walk_rows(So, qr["q"], rows, K, r, T, is_put, betas4)
    up, se, ratio = _pair_mean_se(wk["samples"])
    return dict(upper=up, se_upper=se, se_cancel=ratio, q=qr["q"], samples=wk["samples"],
                inner_path_steps=qr["inner_path_steps"], ties=qr["ties"] + wk["ties"], zmax=wk["zmax"])


def inner_from_normals(Z, So, n_inner, S0_paths):
    """inner(i, t) for upper_bound from the generator's normals Z [N][n_outer (N+1) n_inner/2] (stream_inner, pair offset
    0) and a spot builder S0_paths(z_half [N][n_inner/2], s0) -> [N+1][n_inner] (gbm_paths_from_normals of the device or
    of the C oracle): pair j of item (i, t) is generator pair (i (N+1) + t) n_inner/2 + j."""
    N = So.shape[0] - 1
    H = n_inner // 2

    def inner(i, t):
        g0 = (i * (N + 1) + t) * H
        return S0_paths(np.ascontiguousarray(Z[:, g0:g0 + H]), float(So[t, i]))[:N - t + 1]

    return inner


def inner_by_item(normals, So, n_inner, S0_paths):
    """inner(i, t) as inner_from_normals gives it, with every item's normals generated on their own: normals(pair_offset,
    n_pairs) -> [N][n_pairs] of stream_inner (gbm_normals of the device or of the C oracle), asked for at pair offset
    (i (N+1) + t) n_inner/2.  No array over the whole call: serves a few sampled outer paths of a large one."""
    N = So.shape[0] - 1
    H = n_inner // 2

    def inner(i, t):
        z = normals((i * (N + 1) + t) * H, H)
        return S0_paths(np.ascontiguousarray(z), float(So[t, i]))[:N - t + 1]

    return inner


def samples_atol(N, q, zmax):
    """Absolute tolerance of a sample max_t (Z_t - M^_t) between two float64 evaluations whose Q^ agree to 1e-12
    relative: M^_t adds 2 t values of Q^ / Z, each within 1e-12 of the largest of them."""
    return 2 * N * 1e-12 * max(float(np.max(q, initial=0.0)), zmax)

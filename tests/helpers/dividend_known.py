"""Known answers for options on a stock that pays proportional dividends, in float64.  TEST
INFRASTRUCTURE ONLY.

  european_proportional   a European option with proportional dividends delta_i and a yield q is Black-Scholes at
                          S0 prod(1 - delta_i) with the yield q: the dividends scale the terminal spot
  bermudan_call_one_proportional
                          a call with q = 0, r >= 0 and one proportional dividend delta on step k >= 2 of the grid.  Between
                          dividends a call is never exercised early, and after the last one it is European, so the holder
                          decides once, at t_{k-1}, the last cum-dividend date: exercise for S - K or keep a European call on
                          S (1 - delta).  V = e^{-r t_{k-1}} E[max(S - K, BS(S (1 - delta), K, T - t_{k-1}))], S lognormal at
                          t_{k-1}, by quadrature over the normal density
  lattice_call_one_proportional
                          the same game on a recombining binomial lattice with m steps per grid interval and exercise at the
                          grid dates only; a proportional dividend keeps the lattice recombining
"""
from __future__ import annotations

import math

import numpy as np


def _ncdf(x):
    return 0.5 * (1.0 + np.vectorize(math.erf)(np.asarray(x, np.float64) / math.sqrt(2.0)))


def black_scholes(S, K, r, q, sigma, tau, is_put):
    """Black-Scholes with a continuous yield q; S may be an array"""
    S = np.asarray(S, np.float64)
    sq = sigma * math.sqrt(tau)
    d1 = (np.log(S / K) + (r - q + 0.5 * sigma * sigma) * tau) / sq
    d2 = d1 - sq
    call = S * math.exp(-q * tau) * _ncdf(d1) - K * math.exp(-r * tau) * _ncdf(d2)
    return call - S * math.exp(-q * tau) + K * math.exp(-r * tau) if is_put else call


def european_proportional(S0, K, r, q, sigma, T, deltas, is_put):
    return float(black_scholes(S0 * float(np.prod([1.0 - d for d in deltas])), K, r, q, sigma, T, is_put))


def normal_mean(f, n=100_001, width=10.0):
    """E[f(X)], X standard normal, by the trapezoid rule on [-width, width]: the integrands here have a kink, where a
    Gauss-Hermite rule converges like 1 / nodes and a fine uniform grid like h^2"""
    x = np.linspace(-width, width, n)
    y = f(x) * np.exp(-0.5 * x * x)
    return float((np.sum(y) - 0.5 * (y[0] + y[-1])) * (x[1] - x[0]) / math.sqrt(2.0 * math.pi))


def bermudan_call_one_proportional(S0, K, r, sigma, T, N, k, delta, n=100_001):
    assert 2 <= k <= N and r >= 0.0
    t1 = (k - 1) * T / N

    def value(x):
        S = S0 * np.exp((r - 0.5 * sigma * sigma) * t1 + sigma * math.sqrt(t1) * x)
        return np.maximum(S - K, black_scholes(S * (1.0 - delta), K, r, 0.0, sigma, T - t1, False))

    return math.exp(-r * t1) * normal_mean(value, n)


def lattice_call_one_proportional(S0, K, r, sigma, T, N, k, delta, m):
    """CRR lattice of N m steps; exercise at steps j m, j = 1 .. N, on the ex-dividend spot from grid date k on"""
    n = N * m
    dt = T / n
    u = math.exp(sigma * math.sqrt(dt))
    d = 1.0 / u
    pu = (math.exp(r * dt) - d) / (u - d)
    disc = math.exp(-r * dt)

    def spots(step):
        j = np.arange(step + 1)
        return S0 * u ** j * d ** (step - j) * ((1.0 - delta) if step >= k * m else 1.0)

    V = np.maximum(spots(n) - K, 0.0)
    for step in range(n - 1, 0, -1):
        V = disc * (pu * V[1:] + (1.0 - pu) * V[:-1])
        if step % m == 0:
            V = np.maximum(V, spots(step) - K)
    return float(disc * (pu * V[1] + (1.0 - pu) * V[0]))


def bermudan_one_dividend_grid(S0, K, r, sigma, T, N, k, amount, kind, is_put, q=0.0, m=1500, nz=1201):
    """(c): the Bermudan value on the grid (exercise at t = 1 .. N on the ex-dividend spot of the date) of a put or call with
    one dividend on step k, cash or proportional, by float64 backward induction on a uniform log-spot grid of m points:
    V_N = payoff, C_t(s) = e^{-r dt} E[V_{t+1}(g_{t+1}(s e^{a + b z}))] with g the dividend map of step t + 1 (the identity
    elsewhere), the expectation by the trapezoid rule over nz points of z, V_{t+1} interpolated linearly in log s; a spot of
    exactly 0 (a cash dividend larger than the spot) is carried beside the grid: it stays 0"""
    dt = T / N
    a, b = (r - q - 0.5 * sigma * sigma) * dt, sigma * math.sqrt(dt)
    w = 10.0 * sigma * math.sqrt(T) + abs(r - q) * T + 1.0
    x = np.linspace(math.log(S0) - w, math.log(S0) + w, m)
    s = np.exp(x)
    z = np.linspace(-9.0, 9.0, nz)
    pz = np.exp(-0.5 * z * z)
    pz[[0, -1]] *= 0.5
    pz *= (z[1] - z[0]) / math.sqrt(2.0 * math.pi)
    disc = math.exp(-r * dt)

    def pay(v):
        return np.maximum(K - v if is_put else v - K, 0.0)

    def after(v, step):
        if step != k:
            return v
        return np.maximum(v * (1.0 - amount), 0.0) if kind == "proportional" else np.maximum(v - amount, 0.0)

    V, V0 = pay(s), float(pay(np.float64(0.0)))  # the value on the grid and at a spot of exactly 0
    for t in range(N - 1, -1, -1):
        nxt = after(np.exp(x[:, None] + a + b * z[None, :]), t + 1)  # [m][nz] ex-dividend spots of date t + 1
        val = np.where(nxt > 0.0, np.interp(np.log(np.maximum(nxt, 1e-300)), x, V), V0)
        C, C0 = disc * (val @ pz), disc * V0
        if t == 0:
            return float(np.interp(math.log(S0), x, C))
        V, V0 = np.maximum(pay(s), C), max(float(pay(np.float64(0.0))), C0)

"""Bermudan lattices for the multi-asset bound tests (omc_price_american_basket_bounds).  TEST
INFRASTRUCTURE ONLY.

two_asset   the Boyle-Evnine-Gibbs (1989) binomial lattice of two correlated GBM assets with continuous yields: per step h
            each asset moves by exp(+-sigma_i sqrt(h)), the four joint moves have the probabilities
                p(+-, +-) = (1 + s1 s2 rho + sqrt(h) (s1 mu_1 / sigma_1 + s2 mu_2 / sigma_2)) / 4,   mu_i = r - q_i - sigma_i^2 / 2,
            and the option on the index (arithmetic w_1 S_1 + w_2 S_2, best-of max, worst-of min of the w_i S_i) may be
            exercised every m-th step: n_dates dates, the game of the bounds (dates t = 1 .. N, none at 0).
one_asset   the Cox-Ross-Rubinstein lattice of one asset with a yield and the same dates.
Both return the value at t = 0 discounted with r.  Their error falls like 1 / m; tests compare two resolutions.
"""
from __future__ import annotations

import math

import numpy as np

KINDS = ("basket", "best-of", "worst-of")


def _index(kind, x1, x2):
    if kind in ("basket", "arithmetic"):
        return x1 + x2
    if kind == "best-of":
        return np.maximum(x1, x2)
    if kind == "worst-of":
        return np.minimum(x1, x2)
    raise ValueError(f"kind must be one of {KINDS}.")


def two_asset(S0, K, r, sigmas, T, n_dates, m, yields=(0.0, 0.0), rho=0.0, weights=(1.0, 1.0), kind="best-of",
              is_put=False):
    """Value of the Bermudan option on the index of two assets: S0, sigmas, yields, weights are pairs; n_dates exercise
    dates T k / n_dates, m lattice steps between two of them."""
    n = n_dates * m
    h = T / n
    sh = math.sqrt(h)
    (s1, s2), (q1, q2), (w1, w2) = sigmas, yields, weights
    m1, m2 = (r - q1 - 0.5 * s1 * s1) / s1, (r - q2 - 0.5 * s2 * s2) / s2
    puu, pud = 0.25 * (1 + rho + sh * (m1 + m2)), 0.25 * (1 - rho + sh * (m1 - m2))
    pdu, pdd = 0.25 * (1 - rho + sh * (m2 - m1)), 0.25 * (1 + rho - sh * (m1 + m2))
    if min(puu, pud, pdu, pdd) < 0.0:
        raise ValueError("the step is too coarse for these parameters (a negative probability).")
    disc = math.exp(-r * h)

    def payoff(k):  # at step k: node (i, j) has i / j up moves of asset 1 / 2
        up = 2.0 * np.arange(k + 1) - k
        x1 = (w1 * S0[0]) * np.exp(s1 * sh * up)[:, None]
        x2 = (w2 * S0[1]) * np.exp(s2 * sh * up)[None, :]
        X = _index(kind, x1, x2)
        return np.maximum(K - X, 0.0) if is_put else np.maximum(X - K, 0.0)

    V = payoff(n)
    for k in range(n - 1, -1, -1):
        V = disc * (puu * V[1:, 1:] + pud * V[1:, :-1] + pdu * V[:-1, 1:] + pdd * V[:-1, :-1])
        if k > 0 and k % m == 0:
            V = np.maximum(V, payoff(k))
    return float(V[0, 0])


def one_asset(S0, K, r, sigma, T, n_dates, m, q=0.0, is_put=False):
    """Value of the Bermudan option on one asset with a continuous yield q (Cox-Ross-Rubinstein, the same dates)."""
    n = n_dates * m
    h = T / n
    u = math.exp(sigma * math.sqrt(h))
    p = (math.exp((r - q) * h) - 1.0 / u) / (u - 1.0 / u)
    if not 0.0 <= p <= 1.0:
        raise ValueError("the step is too coarse for these parameters (a probability outside [0, 1]).")
    disc = math.exp(-r * h)

    def payoff(k):
        S = S0 * np.exp(sigma * math.sqrt(h) * (2.0 * np.arange(k + 1) - k))
        return np.maximum(K - S, 0.0) if is_put else np.maximum(S - K, 0.0)

    V = payoff(n)
    for k in range(n - 1, -1, -1):
        V = disc * (p * V[1:] + (1.0 - p) * V[:-1])
        if k > 0 and k % m == 0:
            V = np.maximum(V, payoff(k))
    return float(V[0])

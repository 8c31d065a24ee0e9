"""Barrier-option references (omc_price_barrier; conventions in include/omc.h and DESIGN.md section 11).  TEST
INFRASTRUCTURE ONLY.

- closed forms of the 8 continuously monitored European barriers under GBM, no rebate, no dividend (Merton 1973,
  Reiner & Rubinstein 1991, in the A..D notation of Haug, "The Complete Guide to Option Pricing Formulas");
- the encoder that applies the library's conventions to a host path matrix: a knock-out is dead AT its hit step, a
  knock-in is live FROM its hit step (row 0 of a knock-in is dead); dead entries hold the dead spot;
- a numpy restatement of the device's continuous-monitoring hit steps (Brownian-bridge test on the documented Philox
  counters) and a plain numpy Brownian-bridge Monte Carlo.
"""
from __future__ import annotations

import math

import numpy as np

KINDS = ("down-and-out", "up-and-out", "down-and-in", "up-and-in")
L2E = 1.4426950408889634074


def _ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def black_scholes(S, K, r, sigma, T, is_put):
    sq = sigma * math.sqrt(T)
    d1 = (math.log(S / K) + (r + 0.5 * sigma * sigma) * T) / sq
    d2 = d1 - sq
    if is_put:
        return K * math.exp(-r * T) * _ncdf(-d2) - S * _ncdf(-d1)
    return S * _ncdf(d1) - K * math.exp(-r * T) * _ncdf(d2)


def closed_form(kind, is_put, S, K, H, r, sigma, T):
    """Continuously monitored European barrier option under GBM (cost of carry r), no rebate.  S must lie on the live
    side of H."""
    down = kind.startswith("down")
    knock_in = kind.endswith("-in")
    if (down and S <= H) or (not down and S >= H):
        raise ValueError("S on or beyond the barrier")
    phi = -1.0 if is_put else 1.0
    eta = 1.0 if down else -1.0
    sq = sigma * math.sqrt(T)
    mu = (r - 0.5 * sigma * sigma) / (sigma * sigma)
    dK = K * math.exp(-r * T)
    x1 = math.log(S / K) / sq + (1 + mu) * sq
    x2 = math.log(S / H) / sq + (1 + mu) * sq
    y1 = math.log(H * H / (S * K)) / sq + (1 + mu) * sq
    y2 = math.log(H / S) / sq + (1 + mu) * sq
    hs1, hs0 = (H / S) ** (2 * (mu + 1)), (H / S) ** (2 * mu)
    A = phi * S * _ncdf(phi * x1) - phi * dK * _ncdf(phi * x1 - phi * sq)
    B = phi * S * _ncdf(phi * x2) - phi * dK * _ncdf(phi * x2 - phi * sq)
    C = phi * S * hs1 * _ncdf(eta * y1) - phi * dK * hs0 * _ncdf(eta * y1 - eta * sq)
    D = phi * S * hs1 * _ncdf(eta * y2) - phi * dK * hs0 * _ncdf(eta * y2 - eta * sq)
    above = K > H
    if not is_put:
        if down:
            v_in = C if above else A - B + D
            v_out = A - C if above else B - D
        else:
            v_in = A if above else B - C + D
            v_out = 0.0 if above else A - B + C - D
    else:
        if down:
            v_in = B - C + D if above else A
            v_out = A - B + C - D if above else 0.0
        else:
            v_in = A - B + D if above else C
            v_out = B - D if above else A - C
    return v_in if knock_in else v_out


def dead_spot(K, is_put):
    """The float32 nearest to K on its out-of-the-money side (the sweeps' in-the-money threshold)."""
    Kf = np.float32(K)
    if is_put:
        return np.nextafter(Kf, np.float32(np.inf)) if float(Kf) < K else Kf
    return np.nextafter(Kf, np.float32(-np.inf)) if float(Kf) > K else Kf


def discrete_hit_steps(S_full, kind, H):
    """First step t in 1..N at which (double)S_t <= H (down) / >= H (up), per column; N + 1 where it never hits."""
    S = np.asarray(S_full, np.float32).astype(np.float64)
    N = S.shape[0] - 1
    hit = S[1:] <= H if kind.startswith("down") else S[1:] >= H
    first = np.where(hit.any(axis=0), hit.argmax(axis=0) + 1, N + 1)
    return first.astype(np.int64)


def encode(S_full, kind, H, hit_steps=None, K=100.0, is_put=True):
    """The matrix omc_price_barrier hands to the LSM sweeps: the real spot where the option is live, dead_spot(K) where
    it is not.  hit_steps (per column, N + 1 = never) defaults to the discrete test."""
    S = np.array(S_full, np.float32, copy=True)
    N = S.shape[0] - 1
    if hit_steps is None:
        hit_steps = discrete_hit_steps(S, kind, H)
    t = np.arange(N + 1)[:, None]
    hs = np.asarray(hit_steps)[None, :]
    dead_mask = t < hs if kind.endswith("-in") else t >= hs
    S[dead_mask] = dead_spot(K, is_put)
    return S


def bridge_uniforms(n_pairs, n_steps, seed, stream=0, pair_offset=0):
    """u [n_steps][n_pairs] float32: u_t of the crossing test of step t+1, from the documented Philox counters
    (pair lo, pair hi, 0x80000000 | (t >> 2), stream), word t & 3, u = (w >> 8) 2^-24."""
    from oracle import cpu as orc
    nb = (n_steps + 3) // 4
    u = np.empty((nb * 4, n_pairs), np.float32)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for p in range(n_pairs):
        g = pair_offset + p
        for blk in range(nb):
            o = orc.philox4x32_10((g & 0xFFFFFFFF, g >> 32, 0x80000000 | blk, stream & 0xFFFFFFFF), key)
            u[4 * blk:4 * blk + 4, p] = (o >> 8).astype(np.float32) * np.float32(2.0 ** -24)
    return u[:n_steps]


def bridge_probabilities(Z, S0, H, r, sigma, T):
    """The device's crossing probabilities p [N][2P] (float64 of the float32 restatement) for both partners of every
    pair (columns: first partners, then their antithetic partners) from the pair normals Z [N][P]:
    x_0 = f32(log2(f32(S0) / H)), x_t = x_{t-1} + f32(a +- b z_t), p_t = exp2((c x_{t-1}) x_t)."""
    N, P = Z.shape
    dt = T / N
    a = np.float32((r - 0.5 * sigma * sigma) * dt * L2E)
    b = np.float32(sigma * math.sqrt(dt) * L2E)
    c = np.float32(-2.0 * math.log(2.0) / (sigma * sigma * dt))
    x0 = np.float32(math.log2(float(np.float32(S0)) / H))
    z = np.asarray(Z, np.float32).astype(np.float64)
    inc = np.concatenate([(np.float64(b) * z + np.float64(a)).astype(np.float32),
                          (np.float64(-b) * z + np.float64(a)).astype(np.float32)], axis=1)  # the fma, rounded once
    x = np.empty((N + 1, 2 * P), np.float32)
    x[0] = x0
    for t in range(N):
        x[t + 1] = x[t] + inc[t]
    return np.exp2(((c * x[:-1]).astype(np.float32) * x[1:]).astype(np.float32).astype(np.float64))


def continuous_hit_steps(S_full, Z, u, S0, H, r, sigma, T, kind):
    """-> (hit steps [2P] (N + 1 = never), |u - p| [N][2P]): the discrete test on the spots S_full [N+1][2P] or the
    bridge test u_t < p_t, whichever comes first."""
    N = S_full.shape[0] - 1
    prob = bridge_probabilities(Z, S0, H, r, sigma, T)
    uu = np.concatenate([u, u], axis=1).astype(np.float64)
    S = np.asarray(S_full, np.float32).astype(np.float64)
    spot = S[1:] <= H if kind.startswith("down") else S[1:] >= H
    hit = spot | (uu < prob)
    first = np.where(hit.any(axis=0), hit.argmax(axis=0) + 1, N + 1)
    return first.astype(np.int64), np.abs(uu - prob)


def bridge_mc(kind, is_put, S0, K, H, r, sigma, T, n_paths, n_steps, seed=0):
    """Plain numpy Monte Carlo of the continuously monitored option: exact GBM on the grid plus the Brownian-bridge
    crossing test between grid points -> (price, standard error)."""
    rng = np.random.default_rng(seed)
    dt = T / n_steps
    down = kind.startswith("down")
    lnH = math.log(H)
    x = np.full(n_paths, math.log(S0))
    hit = np.zeros(n_paths, bool)
    for _ in range(n_steps):
        xn = x + (r - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * rng.standard_normal(n_paths)
        crossed = (xn <= lnH) if down else (xn >= lnH)
        p = np.exp(-2.0 * (x - lnH) * (xn - lnH) / (sigma * sigma * dt))
        hit |= crossed | (rng.random(n_paths) < np.where(crossed, 1.0, p))
        x = xn
    ST = np.exp(x)
    pay = np.maximum(K - ST, 0.0) if is_put else np.maximum(ST - K, 0.0)
    v = np.where(hit, pay, 0.0) if kind.endswith("-in") else np.where(hit, 0.0, pay)
    v *= math.exp(-r * T)
    return float(v.mean()), float(v.std() / math.sqrt(n_paths))

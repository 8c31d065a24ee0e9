"""numpy restatement of the jump-diffusion semantics (include/omc.h).  TEST INFRASTRUCTURE ONLY.

table()     kappa, the drift rate and the 16 Poisson thresholds of a step (what omc_jump_table returns), in float64 with
            the C library's exp (math.exp), in the order the header states.
count()     the integer rule: n = #{k : w >= thr[k]}.
draws()     counts and jump normals of every (step, pair) from Philox blocks: counts from the top 24 bits of the count
            block's words, z_J = sqrt(-2 ln u1) cos(2 pi u2) in float64 with box_muller's u1, u2.  `philox` is any
            function (counter[4], key[2]) -> four uint32 (the tests pass the C oracle's).
apply()     the matrix with jumps from a VANILLA matrix at the drift rate rj, whatever the model: the vanilla generator's
            own growth factors V_t / V_{t-1}, re-applied in float64, times exp(J_t), J_t = n mu_j + sqrt(n) sigma_j z_J, the
            same for both partners of a pair (columns p and p + P).  As in dividend_ref each ratio of two float32 spots
            carries up to 2^-23 of rounding, so the tests keep N <= 64 and use dividend_ref.close.
merton()    Merton's series for a European option under jump-diffusion with a continuous yield.
"""
import math

import numpy as np

from helpers import dividend_ref as dr

N_THR = 16
TWO24 = 1 << 24
COUNT_TAG, SIZE_TAG = 0x40000000, 0xC0000000


def table(lam, mu_j, sigma_j, r, q, T, n_steps):
    """-> (thr uint32 [16], kappa, drift_rate, n_thresholds: entries below 2^24)"""
    kappa = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0
    rate = (r - q) - lam * kappa
    x = lam * T / n_steps
    thr = np.empty(N_THR, np.uint32)
    p = math.exp(-x)
    c = 0.0
    for n in range(N_THR):
        if n > 0:
            p = p * x / n
        c += p
        thr[n] = min(TWO24, int(math.floor(c * TWO24 + 0.5)))
    return thr, kappa, rate, int((thr < TWO24).sum())


def count(w, thr):
    """w: the top 24 bits of count words (any shape) -> the number of jumps"""
    w = np.asarray(w, np.int64)
    return (w[..., None] >= np.asarray(thr, np.int64)).sum(axis=-1)


def draws(philox, n_pairs, n_steps, seed, stream, pair_offset, thr):
    """-> (n int64 [N+1][P], zJ float64 [N+1][P]; row 0 and cells without a jump hold 0)"""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    ncb = (n_steps + 3) // 4
    words = np.zeros((n_pairs, 4 * ncb + 1), np.int64)  # [p][t], t = 1 .. 4 ncb
    for p in range(n_pairs):
        pair = pair_offset + p
        lo, hi = pair & 0xFFFFFFFF, (pair >> 32) & 0xFFFFFFFF
        for cb in range(ncb):
            words[p, 4 * cb + 1:4 * cb + 5] = philox((lo, hi, COUNT_TAG | cb, stream), key)
    n = count(words.T[:n_steps + 1] >> 8, thr)
    n[0] = 0
    z = np.zeros((n_steps + 1, n_pairs))
    for t, p in zip(*np.nonzero(n)):
        pair = pair_offset + int(p)
        o = philox((pair & 0xFFFFFFFF, (pair >> 32) & 0xFFFFFFFF, SIZE_TAG | int(t), stream), key)
        u1 = ((int(o[0]) >> 8) + 0.5) / TWO24
        u2 = (int(o[1]) >> 8) / TWO24
        z[t, p] = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
    return n, z


def apply(V, n, zJ, mu_j, sigma_j):
    """V [N+1][2P] vanilla spots at rate rj, n / zJ [N+1][P] -> float64 [N+1][2P] with the jumps applied"""
    V = np.asarray(V, np.float64)
    J = n * mu_j + np.sqrt(n) * sigma_j * zJ
    J = np.concatenate([J, J], axis=1)
    out = np.empty_like(V)
    out[0] = V[0]
    for t in range(1, V.shape[0]):
        with np.errstate(invalid="ignore", divide="ignore"):
            out[t] = out[t - 1] * (V[t] / V[t - 1]) * np.exp(J[t])
    return out


def first_jump_step(n):
    """per pair: the first step with a jump (N + 1: none)"""
    has = n > 0
    return np.where(has.any(axis=0), has.argmax(axis=0), n.shape[0])


def merton(S0, K, r, q, sigma, T, lam, mu_j, sigma_j, is_put, terms=60):
    """sum_n Pois(lam T; n) BSM(S0 exp(-lam kappa T + n (mu_j + sigma_j^2 / 2)), K, r, q, sqrt(sigma^2 + n sigma_j^2 / T), T)"""
    kappa = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0
    total, w = 0.0, math.exp(-lam * T)
    for n in range(terms):
        if n > 0:
            w = w * lam * T / n
        s = S0 * math.exp(-lam * kappa * T + n * (mu_j + sigma_j * sigma_j / 2.0))
        total += w * dr.bsm(s, K, r, q, math.sqrt(sigma * sigma + n * sigma_j * sigma_j / T), T, is_put)
    return total

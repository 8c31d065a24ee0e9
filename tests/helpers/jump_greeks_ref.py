"""numpy float64 restatement of the frozen-policy Greeks of American options under jump-diffusion
(omc_price_american_jump_greeks; the definitions are in include/omc_jump_greeks.h and DESIGN.md section 34).
TEST INFRASTRUCTURE ONLY.

It works on the three scenario matrices [N+1][M] (base, S0 (1 + h), S0 (1 - h); the partners of pairs 0 .. M/2-1 are
columns M/2 .. M-1), the generator's normals Z [N][M/2], the integer jump counts n and jump normals zJ [N+1][M/2] of
helpers/jump_ref.draws (draws() below is the same thing a pair count at a time, for the large case) and a table of fits
betas4 [N+1][4] = b0, b1, b2, n (n > 0.5 fits).  Stops come from helpers/dividend_greeks_ref.stops: the LATEST fire.
The spot is multiplicative in S0 and in every step's factor, so every pathwise term is the spot at the stop times a sum
up to the stop:  W_k = sqrt(dt) sum z,  Nc_k = sum n,  ZJ_k = sum sqrt(n) zJ;  the score terms take the whole path's
count N_tot.

simulate() draws float64 paths of the law for the self-checks of tests/test_jump_greeks_cpu.py.
"""
from __future__ import annotations

import math

import numpy as np

from helpers import dividend_greeks_ref as dg
from helpers import jump_ref as jr

GREEKS = ("delta", "gamma", "vega", "rho", "theta", "epsilon", "dlambda", "dmu_j", "dsigma_j", "theta_score")
stops, frozen_price, signed = dg.stops, dg.frozen_price, dg.signed


def draws(philox_words, n_pairs, n_steps, seed, stream, pair_offset, thr):
    """jump_ref.draws with the Philox blocks of all pairs at once: philox_words(n_pairs, pair0, c2, stream, seed) ->
    uint32 [n_pairs][4] (the C oracle's).  -> (n int64 [N+1][P], zJ float64 [N+1][P]; row 0 and cells without a jump 0)"""
    n = np.zeros((n_steps + 1, n_pairs), np.int64)
    for cb in range((n_steps + 3) // 4):
        W = philox_words(n_pairs, pair_offset, jr.COUNT_TAG | cb, stream, seed).astype(np.int64) >> 8
        for i in range(4):
            t = 4 * cb + 1 + i
            if t <= n_steps:
                n[t] = jr.count(W[:, i], thr)
    z = np.zeros((n_steps + 1, n_pairs))
    for t in range(1, n_steps + 1):
        if not n[t].any():
            continue
        O = philox_words(n_pairs, pair_offset, jr.SIZE_TAG | t, stream, seed).astype(np.int64)
        u1 = ((O[:, 0] >> 8) + 0.5) / jr.TWO24
        u2 = (O[:, 1] >> 8) / jr.TWO24
        z[t] = np.where(n[t] > 0, np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2), 0.0)
    return n, z


def simulate(S0, r, q, sigma, T, N, Z, n, zJ, lam, mu_j, sigma_j):
    """float64 paths [N+1][2P] of Merton's law on normals Z [N][P], counts n and jump normals zJ [N+1][P]"""
    ZZ = signed(Z)
    dt = T / N
    kappa = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0
    rj = (r - q) - lam * kappa
    J = n * mu_j + np.sqrt(n) * sigma_j * zJ
    J = np.concatenate([J, J], axis=1)
    S = np.empty((N + 1, ZZ.shape[1]))
    S[0] = S0
    for t in range(1, N + 1):
        S[t] = S[t - 1] * np.exp((rj - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * ZZ[t - 1] + J[t])
    return S


def greeks(S3, S0, K, r, q, T, is_put, betas4, h, lam, mu_j, sigma_j, sigma=None, Z=None, n=None, zJ=None, tex3=None):
    """S3 = (S, S_up, S_down).  -> dict: price, sum, sumsq, n_exercised, n_zero, price_up, price_down, n_exercised_up /
    _down, n_jumps, the Greeks and se_* (everything but delta and gamma NaN without Z), `terms` (name -> per-path array),
    `tex` (scenario -> steps) and `ties`.  tex3: exercise steps to hold fixed instead of deciding."""
    S3 = [np.asarray(S, np.float64) for S in S3]
    S = S3[0]
    N, M = S.shape[0] - 1, S.shape[1]
    dt = T / N
    sign = -1.0 if is_put else 1.0
    D = np.exp(-r * dt * np.arange(N + 1))
    cols = np.arange(M)

    def phi(s):
        return K - s if is_put else s - K

    tex, ties = {}, [0, 0, 0]
    for e in range(3):
        tex[e], ties[e] = (np.asarray(tex3[e]), 0) if tex3 is not None else stops(S3[e], K, is_put, betas4)
    k = tex[0]
    s = S[k, cols]
    imm = phi(s)
    Dk = D[k - 1]
    cf = np.maximum(imm, 0.0) * Dk
    Dps = np.where(imm > 0.0, sign, 0.0) * Dk * s
    terms = dict(cf=cf, delta=Dps / S0)
    out = dict(n_jumps=None)
    if Z is not None:
        kappa = math.exp(mu_j + sigma_j * sigma_j / 2.0) - 1.0
        rj = (r - q) - lam * kappa
        zero = np.zeros((1, M))
        W = np.concatenate([zero, math.sqrt(dt) * np.cumsum(signed(Z), axis=0)])[k, cols]  # (the partner's sign inside)
        n2 = np.concatenate([n, n], axis=1).astype(np.float64)
        Nc = np.cumsum(n2, axis=0)
        ZJ = np.cumsum(np.sqrt(n2) * np.concatenate([zJ, zJ], axis=1), axis=0)
        ntot = Nc[N]
        tk = k * dt
        terms["vega"] = Dps * (-sigma * tk + W)
        terms["epsilon"] = -Dps * tk
        terms["rho"] = -(k - 1) * dt * cf + Dps * tk
        terms["dmu_j"] = Dps * (Nc[k, cols] - lam * tk * (kappa + 1.0))
        terms["dsigma_j"] = Dps * (ZJ[k, cols] - lam * tk * sigma_j * (kappa + 1.0))
        terms["dlambda_pathwise"] = Dps * (-kappa * tk)
        score_T = cf * (ntot / T - lam)
        terms["theta_score"] = -score_T
        terms["theta"] = -(-r * (k - 1) / N * cf + Dps * ((rj - 0.5 * sigma * sigma) * k / N + sigma * W / (2.0 * T)) + score_T)
        if lam > 0.0:
            terms["dlambda"] = terms["dlambda_pathwise"] + cf * (ntot / lam - T)
        out["n_jumps"] = int(np.asarray(n).sum())
    dl = []
    for e, name in ((1, "up"), (2, "down")):
        ke = tex[e]
        se = S3[e][ke, cols]
        ie = phi(se)
        De = D[ke - 1]
        terms[name] = np.maximum(ie, 0.0) * De
        # dS/dS0 of a scenario is the product of its growth factors, the same for all three: read from the BASE matrix for
        # both bumped chains.  se / (S0 f) is the same number rounded differently per scenario, and the difference of the two
        # over 2 h S0 is float32 noise of gamma's own size on every path whose bumped chains stop together
        dl.append(np.where(ie > 0.0, sign, 0.0) * De * S[ke, cols] / S[0, cols])
    terms["gamma"] = (dl[0] - dl[1]) / (2.0 * h * S0)
    out.update(terms=terms, ties=ties, n_paths=M, tex=tex)
    out.update(sum=float(cf.sum()), sumsq=float((cf * cf).sum()), price=float(cf.sum() / M),
               n_exercised=int((k < N).sum()), n_zero=int((cf == 0.0).sum()),
               n_exercised_up=int((tex[1] < N).sum()), n_exercised_down=int((tex[2] < N).sum()),
               price_up=float(terms["up"].mean()), price_down=float(terms["down"].mean()))
    out["se_price"] = math.sqrt(max(out["sumsq"] / M - out["price"] ** 2, 0.0) / M)
    for name in GREEKS + ("dlambda_pathwise",):
        if name in terms:
            x = terms[name]
            m = float(x.mean())
            out[name] = m
            out["se_" + name] = math.sqrt(max(float((x * x).mean()) - m * m, 0.0) / M)
        else:
            out[name] = out["se_" + name] = float("nan")
    return out

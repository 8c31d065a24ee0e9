"""numpy float64 restatement of the frozen-policy Greeks of American options on a dividend-paying stock
(omc_price_american_div_greeks; the definitions are in include/omc_dividend_greeks.h and DESIGN.md section 32).
TEST INFRASTRUCTURE ONLY.

It works on the three scenario matrices [N+1][M] (base, S0 (1 + h), S0 (1 - h); the partners of pairs 0 .. M/2-1 are
columns M/2 .. M-1), the per-step dividend table (helpers/dividend_ref.schedule) and a table of fits betas4 [N+1][4] =
b0, b1, b2, n (n > 0.5 fits), with the decision rule of helpers/greeks_ref.py.

  * The S0 tangent comes from the matrix ALONE, by a formula that is not the kernel's recurrence:
        Y_k = (S_k / S_0) * prod over cash-dividend rows j <= k of (1 + c_j / S_j),   0 from the first row whose spot is 0.
    (At a row with S_j = m S^- - c > 0: Y_j / S_j = m Y^- / S_j = (Y^- / S^-) (S_j + c) / S_j.)  It serves every model.
  * The GBM tangents Ys, Yr, YT follow the recurrence of the definition in float64 on the generator's normals Z [N][M/2].

simulate() draws float64 paths of the law for the self-check of tests/test_dividend_greeks_cpu.py.
"""
from __future__ import annotations

import math

import numpy as np

TIE = 1e-10  # decision margins |imm - cont| <= TIE * K count as ties (either branch is worth the same)
GREEKS = ("delta", "gamma", "vega", "rho", "theta", "epsilon")


def signed(Z):
    """Z [N][P] -> [N][2P]: the partners take -Z"""
    Z = np.asarray(Z, np.float64)
    return np.concatenate([Z, -Z], axis=1)


def simulate(S0, r, q, sigma, T, N, Z, mul, cash, has, alive=None):
    """float64 paths [N+1][2P] of the dividend law on normals Z [N][P]; alive [N+1][2P] (bool), when given, replaces the
    floor's own test: s = m s - c where alive, 0 elsewhere (the frozen-decision price of the self-check)"""
    ZZ = signed(Z)
    dt = T / N
    S = np.empty((N + 1, ZZ.shape[1]))
    S[0] = S0
    for t in range(1, N + 1):
        s = S[t - 1] * np.exp((r - q - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * ZZ[t - 1])
        if has[t]:
            x = s * float(mul[t]) - float(cash[t])
            s = np.maximum(x, 0.0) if alive is None else np.where(alive[t], x, 0.0)
        S[t] = s
    return S


def s0_tangent(S, cash, has):
    """dS_k / dS_0 [N+1][M] from the matrix alone"""
    S = np.asarray(S, np.float64)
    Y = np.empty_like(S)
    prod = np.ones(S.shape[1])
    dead = np.zeros(S.shape[1], bool)
    for k in range(S.shape[0]):
        dead |= S[k] == 0.0
        if has[k] and float(cash[k]) != 0.0:
            with np.errstate(divide="ignore", invalid="ignore"):
                prod = np.where(dead, 0.0, prod * (1.0 + float(cash[k]) / S[k]))
        Y[k] = np.where(dead, 0.0, S[k] / S[0] * prod)
    return Y


def gbm_tangents(S, r, q, sigma, T, Z, mul, has):
    """(Ys, Yr, YT) [N+1][M]: dS_k/dsigma, dS_k/dr (= -dS_k/dq), dS_k/dT at fixed N, by the recurrence, float64"""
    S = np.asarray(S, np.float64)
    N = S.shape[0] - 1
    ZZ = signed(Z)
    dt = T / N
    mu = r - q - 0.5 * sigma * sigma
    Ys, Yr, YT = (np.zeros_like(S) for _ in range(3))
    for t in range(1, N + 1):
        z = ZZ[t - 1]
        G = np.exp(mu * dt + sigma * math.sqrt(dt) * z)
        Sm = S[t - 1] * G  # the cum-dividend spot
        ys = Ys[t - 1] * G + Sm * (-sigma * dt + math.sqrt(dt) * z)
        yr = Yr[t - 1] * G + Sm * dt
        yT = YT[t - 1] * G + Sm * (mu / N + sigma * z / (2.0 * math.sqrt(T * N)))
        if has[t]:
            m = np.where(S[t] > 0.0, float(mul[t]), 0.0)
            ys, yr, yT = m * ys, m * yr, m * yT
        Ys[t], Yr[t], YT[t] = ys, yr, yT
    return Ys, Yr, YT


def stops(S, K, is_put, betas4):
    """-> (exercise step [M]: the LATEST step in 1 .. N-1 at which the rule fires, N where none; ties): the frozen-fit rule
    of helpers/greeks_ref.py, walking backward as it does"""
    S = np.asarray(S, np.float64)
    N, M = S.shape[0] - 1, S.shape[1]
    b = np.asarray(betas4, np.float64)
    tex = np.full(M, N, np.int64)
    ties = 0
    for t in range(N - 1, 0, -1):
        if not (b[t, 3] > 0.5):
            continue
        s = S[t]
        imm = K - s if is_put else s - K
        u = s * (1.0 / K) - 1.0
        with np.errstate(invalid="ignore", over="ignore"):
            cont = u * (u * b[t, 2] + b[t, 1]) + b[t, 0]
        cand = (tex == N) & (imm > 0.0)
        with np.errstate(invalid="ignore"):
            ties += int(np.count_nonzero(cand & (np.abs(imm - cont) <= TIE * K)))
        tex[cand & (imm > cont)] = t
    return tex, ties


def greeks(S3, K, r, q, T, is_put, betas4, mul, cash, has, h, sigma=None, Z=None, tex3=None):
    """S3 = (S, S_up, S_down).  -> dict: price, sum, sumsq, n_exercised, n_zero, price_up, price_down, n_exercised_up /
    _down, the Greeks and se_* (vega, rho, theta, epsilon NaN without Z), `terms` (name -> per-path array), `tex` (scenario
    -> steps) and `ties`.  tex3: exercise steps to hold fixed instead of deciding."""
    S3 = [np.asarray(S, np.float64) for S in S3]
    S = S3[0]
    N, M = S.shape[0] - 1, S.shape[1]
    S0 = float(S[0, 0])
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
    Dp = np.where(imm > 0.0, sign, 0.0) * Dk
    terms = dict(cf=cf, delta=Dp * s0_tangent(S, cash, has)[k, cols])
    if Z is not None:
        Ys, Yr, YT = gbm_tangents(S, r, q, sigma, T, Z, mul, has)
        terms["vega"] = Dp * Ys[k, cols]
        terms["rho"] = -(k - 1) * dt * cf + Dp * Yr[k, cols]
        terms["epsilon"] = -Dp * Yr[k, cols]
        terms["theta"] = -(-r * (k - 1) / N * cf + Dp * YT[k, cols])
    dl = []
    for e, name in ((1, "up"), (2, "down")):
        ke = tex[e]
        se = S3[e][ke, cols]
        ie = phi(se)
        De = D[ke - 1]
        terms[name] = np.maximum(ie, 0.0) * De
        dl.append(np.where(ie > 0.0, sign, 0.0) * De * s0_tangent(S3[e], cash, has)[ke, cols])
    terms["gamma"] = (dl[0] - dl[1]) / (2.0 * h * S0)
    out = dict(terms=terms, ties=ties, n_paths=M, tex=tex)
    out.update(sum=float(cf.sum()), sumsq=float((cf * cf).sum()), price=float(cf.sum() / M),
               n_exercised=int((k < N).sum()), n_zero=int((cf == 0.0).sum()),
               n_exercised_up=int((tex[1] < N).sum()), n_exercised_down=int((tex[2] < N).sum()),
               price_up=float(terms["up"].mean()), price_down=float(terms["down"].mean()))
    for name in GREEKS:
        if name in terms:
            x = terms[name]
            m = float(x.mean())
            out[name] = m
            out["se_" + name] = math.sqrt(max(float((x * x).mean()) - m * m, 0.0) / M)
        else:
            out[name] = out["se_" + name] = float("nan")
    return out


def frozen_price(S, K, r, T, is_put, tex, itm):
    """the price with the exercise steps AND the in-the-money indicator held fixed: smooth in every parameter"""
    S = np.asarray(S, np.float64)
    N, M = S.shape[0] - 1, S.shape[1]
    s = S[tex, np.arange(M)]
    return float(np.mean(np.exp(-r * (T / N) * (tex - 1)) * np.where(itm, K - s if is_put else s - K, 0.0)))

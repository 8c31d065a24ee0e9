"""numpy restatement of the frozen-policy pathwise Greeks of the two-pass flow (omc_price_american_greeks; the definitions
are in DESIGN.md section 10 and include/omc.h).  TEST INFRASTRUCTURE ONLY.

Works on a host path matrix [N+1][M] (full storage) or on the first partners' half matrix plus the fold table cK
(folded storage: the partner of a stored spot s has moneyness u' = cK[t] / s - 1, spot K (1 + u'), payoff -K u' / K u'),
with a given table of fits betas4 [N+1][4] = b0, b1, b2, n (n > 0.5 fits, as the frozen sweep reads it).
"""
from __future__ import annotations

import math

import numpy as np

TIE = 1e-10  # decision margins |imm - cont| <= TIE * K count as ties (either branch is worth the same)


def betas4_from(betas3, nitm):
    b = np.zeros((len(nitm), 4))
    b[:, :3] = betas3
    b[:, 3] = nitm
    return b


def greeks(S, K, r, T, is_put, betas4, S0, sigma=None, h=0.01, cK=None, gbm=True):
    """-> dict: price, sum, sumsq, n_exercised, n_zero, price_up, price_down, n_exercised_up / _down, delta .. theta and
    se_* (NaN where not gbm), per-path terms `terms` (name -> array over all paths), exercise steps `tex`
    (scenario 0 / 1 / 2 -> array over all paths; folded: stored paths first, then their partners) and `ties`
    (scenario -> number of decisions taken within TIE * K of the continuation value)."""
    S = np.asarray(S, np.float32)
    N, P = S.shape[0] - 1, S.shape[1]
    fold = cK is not None
    b = np.asarray(betas4, np.float64)
    invK = 1.0 / K
    sign = -1.0 if is_put else 1.0
    lam = (1.0, 1.0 + h, 1.0 - h)
    D = np.exp(-r * (T / N) * np.arange(N + 1))

    def phi(s):
        return K - s if is_put else s - K

    parts = (0, 1) if fold else (0,)
    # chains: (part, scenario) -> exercise step [P] and stored spot at it [P]
    tex = {(p, e): np.full(P, N, np.int64) for p in parts for e in range(3)}
    sxs = {(p, e): S[N].copy() for p in parts for e in range(3)}
    ties = [0, 0, 0]
    for t in range(N - 1, 0, -1):
        if not (b[t, 3] > 0.5):
            continue
        b0, b1, b2 = b[t, 0], b[t, 1], b[t, 2]
        row = S[t]
        sd = row.astype(np.float64)
        for p in parts:
            if p == 0:
                base_s, base_imm, base_u = sd, phi(sd), sd * invK - 1.0
            else:
                ub = cK[t] / sd - 1.0
                base_s, base_imm, base_u = K * (1.0 + ub), (-K * ub if is_put else K * ub), ub
            for e in range(3):
                if e == 0:
                    imm, u = base_imm, base_u
                else:
                    ls = lam[e] * base_s
                    imm, u = phi(ls), ls * invK - 1.0
                cont = u * (u * b2 + b1) + b0
                live = tex[(p, e)] == N
                cand = live & (imm > 0.0)
                ties[e] += int(np.count_nonzero(cand & (np.abs(imm - cont) <= TIE * K)))
                ex = cand & (imm > cont)
                tex[(p, e)][ex] = t
                sxs[(p, e)][ex] = row[ex]

    def spot(p, e):
        s = sxs[(p, e)].astype(np.float64)
        if p == 0:
            return s
        return K * (1.0 + (cK[tex[(p, e)]] / s - 1.0))

    cols = {k: [] for k in ("cf", "delta", "gamma", "vega", "rho", "theta", "up", "down")}
    dt = T / N
    for p in parts:
        k = tex[(p, 0)]
        if p == 0:
            s = sxs[(p, 0)].astype(np.float64)
            imm = phi(s)
        else:
            ub = cK[k] / sxs[(p, 0)].astype(np.float64) - 1.0
            imm = -K * ub if is_put else K * ub
            s = K * (1.0 + ub)
        Dk = D[k - 1]
        cf = np.maximum(imm, 0.0) * Dk
        Ds = np.where(imm > 0.0, sign, 0.0) * Dk * s
        cols["cf"].append(cf)
        cols["delta"].append(Ds / S0)
        if gbm:
            tk = k * dt
            lnr = np.log(s / S0)
            cols["vega"].append(Ds * (lnr - (r + 0.5 * sigma * sigma) * tk) / sigma)
            cols["rho"].append(-(k - 1) * dt * cf + Ds * tk)
            cols["theta"].append(-(-r * (k - 1) * dt / T * cf + Ds * (lnr + (r - 0.5 * sigma * sigma) * tk) / (2.0 * T)))
        dl = []
        for e, name in ((1, "up"), (2, "down")):
            ke = tex[(p, e)]
            se = spot(p, e)
            ie = phi(lam[e] * se)
            De = D[ke - 1]
            cols[name].append(np.maximum(ie, 0.0) * De)
            dl.append(np.where(ie > 0.0, sign, 0.0) * De * se / S0)
        cols["gamma"].append((dl[0] - dl[1]) / (2.0 * h * S0))
    terms = {k: np.concatenate(v) for k, v in cols.items() if v}
    M = len(terms["cf"])
    out = dict(terms=terms, ties=ties, n_paths=M,
               tex={e: np.concatenate([tex[(p, e)] for p in parts]) for e in range(3)})
    cf = terms["cf"]
    out.update(sum=float(cf.sum()), sumsq=float((cf * cf).sum()), price=float(cf.sum() / M),
               n_exercised=int((out["tex"][0] < N).sum()), n_zero=int((cf == 0.0).sum()),
               n_exercised_up=int((out["tex"][1] < N).sum()), n_exercised_down=int((out["tex"][2] < N).sum()),
               price_up=float(terms["up"].mean()), price_down=float(terms["down"].mean()))
    for name in ("delta", "gamma", "vega", "rho", "theta"):
        if name in terms:
            x = terms[name]
            m = float(x.mean())
            out[name] = m
            out["se_" + name] = math.sqrt(max(float((x * x).mean()) - m * m, 0.0) / M)
        else:
            out[name] = out["se_" + name] = float("nan")
    return out

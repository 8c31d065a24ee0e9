"""numpy restatement of the frozen-policy pathwise Greeks of the multi-asset options (omc_price_american_basket_greeks; the
definitions are in include/omc.h and DESIGN.md section 19).  TEST INFRASTRUCTURE ONLY.

Works on host asset matrices A [d][N+1][M] and the index matrix X [N+1][M] of the same paths -- float32 as the device
stores them (the float32 products wf_i * s_i are then formed in float32, as the kernel compares them), or float64 for the
CPU checks -- with a table of fits betas4 [N+1][4] = b0, b1, b2, n (n > 0.5 fits) and the law (S0, sigma, q, w, kind).
Everything else is float64.  Chains are walked BACKWARD (the first fire met is the latest one), where the kernel walks
forward and overwrites: the same exercise step.
"""
from __future__ import annotations

import math

import numpy as np

TIE = 1e-10  # decision margins |imm - cont| <= TIE * K count as ties (either branch is worth the same)
KINDS = {"basket": 0, "arithmetic": 0, "geometric": 1, "best-of": 2, "worst-of": 3}


def _mean_se(x):
    m = float(x.mean())
    return m, math.sqrt(max(float((x * x).mean()) - m * m, 0.0) / len(x))


def greeks(A, X, K, r, T, is_put, betas4, S0, sigma, q, w, kind, h=0.01, gamma=True):
    """-> dict: price, sum, sumsq, n_exercised, n_zero; delta, vega, gamma, se_delta, se_vega, se_gamma, price_up,
    price_down, n_exercised_up, n_exercised_down (lists, one entry per asset; the gamma fields are None without `gamma`);
    rho, theta, se_rho, se_theta; `terms` (cf, rho, theta -> array over the paths; delta, vega, gamma, up, down -> list of
    arrays); `tex` (the base chain's exercise steps); `ties` = [base, up, down]: decisions of each chain family taken within
    TIE * K of the continuation value (all assets of a family added)."""
    A = np.asarray(A)
    f32 = A.dtype == np.float32
    d, N1, M = A.shape
    N = N1 - 1
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    Xd = np.asarray(X).astype(np.float64)
    wf = np.asarray(w, np.float32)
    wd = wf.astype(np.float64)
    S0 = [float(x) for x in S0]
    sigma = [float(x) for x in sigma]
    q = [float(x) for x in q]
    b = np.asarray(betas4, np.float64)
    invK = 1.0 / K
    sign = -1.0 if is_put else 1.0
    lam = (1.0 + h, 1.0 - h)
    hw = [(h * wd[i], -h * wd[i]) for i in range(d)]
    cg = [(math.pow(lam[0], wd[i]), math.pow(lam[1], wd[i])) for i in range(d)]
    dt = T / N
    D = np.exp(-r * dt * np.arange(N + 1))
    best = kind == 2
    cols = np.arange(M)

    def phi(x):
        return K - x if is_put else x - K

    def products(rows):
        """rows [d][M] asset spots -> the products the best-of / worst-of index compares, as float64"""
        if f32:
            return [(wf[i] * rows[i]).astype(np.float64) for i in range(d)]
        return [wd[i] * rows[i].astype(np.float64) for i in range(d)]

    def others(P, i):
        m = np.full(M, -np.inf if best else np.inf)
        for j in range(d):
            if j != i:
                m = np.maximum(m, P[j]) if best else np.minimum(m, P[j])
        return m

    def scen_index(i, e, rows, x):
        """the float64 index of scenario (asset i, e = 0 up / 1 down) and its unscaled partial x_i"""
        if kind == 0:
            s = rows[i].astype(np.float64)
            return x + hw[i][e] * s, wd[i] * s
        if kind == 1:
            return x * cg[i][e], wd[i] * x
        P = products(rows)
        m = others(P, i)
        lp = lam[e] * P[i]
        carries = lp >= m if best else lp <= m
        return (np.maximum(lp, m) if best else np.minimum(lp, m)), np.where(carries, P[i], 0.0)

    chains = [("base", 0, 0)] + ([(fam, i, e) for i in range(d) for e, fam in enumerate(("up", "down"))] if gamma else [])
    tex = {c: np.full(M, N, np.int64) for c in chains}
    ties = {"base": 0, "up": 0, "down": 0}
    for t in range(N - 1, 0, -1):
        if not (b[t, 3] > 0.5):
            continue
        b0, b1, b2 = b[t, 0], b[t, 1], b[t, 2]
        rows = A[:, t, :]
        for c in chains:
            fam, i, e = c
            xs = Xd[t] if fam == "base" else scen_index(i, e, rows, Xd[t])[0]
            imm, u = phi(xs), xs * invK - 1.0
            cont = u * (u * b2 + b1) + b0
            cand = (tex[c] == N) & (imm > 0.0)
            ties[fam] += int(np.count_nonzero(cand & (np.abs(imm - cont) <= TIE * K)))
            tex[c][cand & (imm > cont)] = t

    # ---- the base chain's terms
    k = tex[chains[0]]
    rows = A[:, k, cols]  # [d][M]: every asset at the path's own exercise step
    s = rows.astype(np.float64)
    x = Xd[k, cols]
    Dk = D[k - 1]
    imm = phi(x)
    cf = np.maximum(imm, 0.0) * Dk
    Dp = np.where(imm > 0.0, sign, 0.0) * Dk
    tk = k * dt
    if kind == 0:
        xi = [wd[i] * s[i] for i in range(d)]
    elif kind == 1:
        xi = [wd[i] * x for i in range(d)]
    else:
        P = products(rows)
        found = np.zeros(M, bool)
        xi = []
        for i in range(d):
            first = (P[i] == x) & ~found
            found |= first
            xi.append(np.where(first, P[i], 0.0))
    lnr = [np.log(s[i] / S0[i]) for i in range(d)]
    terms = dict(cf=cf, delta=[], vega=[], gamma=[], up=[], down=[])
    sumx = sum(xi)
    sumth = sum(xi[i] * (lnr[i] + (r - q[i] - 0.5 * sigma[i] ** 2) * tk) for i in range(d))
    terms["rho"] = -(k - 1) * dt * cf + Dp * tk * sumx
    terms["theta"] = -(-r * (k - 1) * dt / T * cf + Dp * sumth / (2.0 * T))
    for i in range(d):
        terms["delta"].append(Dp * xi[i] / S0[i])
        terms["vega"].append(Dp * xi[i] * (lnr[i] - (r - q[i] + 0.5 * sigma[i] ** 2) * tk) / sigma[i])
    out = dict(terms=terms, ties=[ties["base"], ties["up"], ties["down"]], tex=k, n_paths=M)
    out.update(sum=float(cf.sum()), sumsq=float((cf * cf).sum()), price=float(cf.sum() / M),
               n_exercised=int((k < N).sum()), n_zero=int((cf == 0.0).sum()))
    for name in ("rho", "theta"):
        out[name], out["se_" + name] = _mean_se(terms[name])
    for name in ("delta", "vega"):
        ms = [_mean_se(v) for v in terms[name]]
        out[name], out["se_" + name] = [m for m, _ in ms], [se for _, se in ms]
    for name in ("gamma", "se_gamma", "price_up", "price_down", "n_exercised_up", "n_exercised_down"):
        out[name] = [] if gamma else None
    if not gamma:
        return out
    # ---- the scenario chains' terms, each at its own exercise step
    for i in range(d):
        dl = []
        for e, fam in enumerate(("up", "down")):
            ke = tex[(fam, i, e)]
            xs, xe = scen_index(i, e, A[:, ke, cols], Xd[ke, cols])
            ie = phi(xs)
            De = D[ke - 1]
            terms[fam].append(np.maximum(ie, 0.0) * De)
            dl.append(np.where(ie > 0.0, sign, 0.0) * De * xe / S0[i])
            out["price_" + fam].append(float(terms[fam][i].mean()))
            out["n_exercised_" + fam].append(int((ke < N).sum()))
        terms["gamma"].append((dl[0] - dl[1]) / (2.0 * h * S0[i]))
        m, se = _mean_se(terms["gamma"][i])
        out["gamma"].append(m)
        out["se_gamma"].append(se)
    return out

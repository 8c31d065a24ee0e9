"""The route the chain's Greeks sweep takes for one entry (omc_price_american_chain_greeks), restated in
numpy.  TEST INFRASTRUCTURE ONLY.

An entry with exercise_every = k is swept on the VIEW of its scheduled rows: view row j = 1 .. Nv is the matrix's row
t(j) = N - k (Nv - j), Nv = (N - 1) // k + 1 (k cut to 2 .. N; below 2: every row, t(j) = j).  The sweep walks the view's rows
Nv-1 .. 1 with the fits, the fold table cv[j] = cK[t(j)] and the valuation table d2[j-1] = D[t(j) - 1] restated on them, keeps
per chain the view row it exercised at (Nv: never), and only then maps that row to its date: tk = t(j) dt, (t(j) - 1) dt and
dt = T / N name the fine grid.  `view_greeks` does exactly that; tests compare it with tests/helpers/greeks_ref.py on the full
matrix under the masked policy -- the route omc_price_american_greeks takes with that policy given -- which must agree.
"""
from __future__ import annotations

import math

import numpy as np

TIE = 1e-10  # as greeks_ref.TIE


def cut(N, k):
    """the schedule as the library cuts it: 1 = every date, else 2 .. N"""
    return min(int(k), N) if k >= 2 else 1


def view_dates(N, k):
    """t(j) for j = 0 .. Nv (t(0) may be below 1: row 0 of a view is never read)"""
    k = cut(N, k)
    Nv = (N - 1) // k + 1
    return np.array([N - k * (Nv - j) for j in range(Nv + 1)], np.int64)


def masked(betas4, k):
    """the policy of the entry on the fine grid: rows at its scheduled dates, zero elsewhere (and at 0 and N)"""
    b = np.asarray(betas4, np.float64)
    N = len(b) - 1
    out = np.zeros_like(b)
    t = view_dates(N, k)[1:-1]
    out[t] = b[t]
    return out


def view_greeks(S, K, r, T, is_put, betas4, S0, sigma=None, h=0.01, every=1, cK=None, gbm=True):
    """S: the matrix [N+1][P] (folded: the first partners, with cK [N+1]); betas4 [N+1][4] on the FINE grid, of which the rows
    at the scheduled dates are read.  -> the dict of greeks_ref.greeks (tex: FINE dates)."""
    S = np.asarray(S, np.float32)
    N, P = S.shape[0] - 1, S.shape[1]
    t_of = view_dates(N, every)
    Nv = len(t_of) - 1
    fold = cK is not None
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    # the tables on the view's rows
    bv = np.zeros((Nv + 1, 4))
    bv[1:Nv] = np.asarray(betas4, np.float64)[t_of[1:Nv]]
    d2 = D[t_of[1:] - 1]                                       # d2[j - 1] values an exercise at view row j
    cv = np.zeros(Nv + 1)
    if fold:
        cv[1:] = np.asarray(cK, np.float64)[t_of[1:]]
    row_of = lambda j: S[t_of[j]]                              # noqa: E731  (view row j, j >= 1)
    invK, sign, lam = 1.0 / K, (-1.0 if is_put else 1.0), (1.0, 1.0 + h, 1.0 - h)

    def phi(s):
        return K - s if is_put else s - K

    parts = (0, 1) if fold else (0,)
    jx = {(p, e): np.full(P, Nv, np.int64) for p in parts for e in range(3)}   # view row of the exercise
    sx = {(p, e): row_of(Nv).copy() for p in parts for e in range(3)}          # stored spot there
    ties = [0, 0, 0]
    for j in range(Nv - 1, 0, -1):
        if not (bv[j, 3] > 0.5):
            continue
        b0, b1, b2 = bv[j, :3]
        row = row_of(j)
        sd = row.astype(np.float64)
        for p in parts:
            if p == 0:
                base_s, base_imm, base_u = sd, phi(sd), sd * invK - 1.0
            else:
                ub = cv[j] / sd - 1.0
                base_s, base_imm, base_u = K * (1.0 + ub), (-K * ub if is_put else K * ub), ub
            for e in range(3):
                if e == 0:
                    imm, u = base_imm, base_u
                else:
                    ls = lam[e] * base_s
                    imm, u = phi(ls), ls * invK - 1.0
                cont = u * (u * b2 + b1) + b0
                cand = (jx[(p, e)] == Nv) & (imm > 0.0)
                ties[e] += int(np.count_nonzero(cand & (np.abs(imm - cont) <= TIE * K)))
                ex = cand & (imm > cont)
                jx[(p, e)][ex] = j
                sx[(p, e)][ex] = row[ex]

    def spot(p, e):
        s = sx[(p, e)].astype(np.float64)
        return s if p == 0 else K * (1.0 + (cv[jx[(p, e)]] / s - 1.0))

    cols = {k: [] for k in ("cf", "delta", "gamma", "vega", "rho", "theta", "up", "down")}
    dt = T / N
    for p in parts:
        j = jx[(p, 0)]
        if p == 0:
            s = sx[(p, 0)].astype(np.float64)
            imm = phi(s)
        else:
            ub = cv[j] / sx[(p, 0)].astype(np.float64) - 1.0
            imm = -K * ub if is_put else K * ub
            s = K * (1.0 + ub)
        Dk = d2[j - 1]
        cf = np.maximum(imm, 0.0) * Dk
        Ds = np.where(imm > 0.0, sign, 0.0) * Dk * s
        cols["cf"].append(cf)
        cols["delta"].append(Ds / S0)
        if gbm:
            k = t_of[j]                                        # the step map: only the times take it
            tk = k * dt
            lnr = np.log(s / S0)
            cols["vega"].append(Ds * (lnr - (r + 0.5 * sigma * sigma) * tk) / sigma)
            cols["rho"].append(-(k - 1) * dt * cf + Ds * tk)
            cols["theta"].append(-(-r * (k - 1) * dt / T * cf + Ds * (lnr + (r - 0.5 * sigma * sigma) * tk) / (2.0 * T)))
        dl = []
        for e, name in ((1, "up"), (2, "down")):
            je = jx[(p, e)]
            se = spot(p, e)
            ie = phi(lam[e] * se)
            De = d2[je - 1]
            cols[name].append(np.maximum(ie, 0.0) * De)
            dl.append(np.where(ie > 0.0, sign, 0.0) * De * se / S0)
        cols["gamma"].append((dl[0] - dl[1]) / (2.0 * h * S0))
    terms = {k: np.concatenate(v) for k, v in cols.items() if v}
    M = len(terms["cf"])
    tex = {e: np.concatenate([t_of[jx[(p, e)]] for p in parts]) for e in range(3)}
    out = dict(terms=terms, ties=ties, n_paths=M, tex=tex)
    cf = terms["cf"]
    out.update(sum=float(cf.sum()), sumsq=float((cf * cf).sum()), price=float(cf.sum() / M),
               n_exercised=int((tex[0] < N).sum()), n_zero=int((cf == 0.0).sum()),
               n_exercised_up=int((tex[1] < N).sum()), n_exercised_down=int((tex[2] < N).sum()),
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


# ------------------------------------------------------------------ seeded cases of tests/test_gpu_chain_greeks_fuzz.py
HESTON = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)


def fuzz_cases(n, seed):
    """Random chains: 1 .. 70 steps, ragged even path counts on both storages, 1 .. 20 entries with random sides, strikes within
    +-30 % of the spot and schedules 0 .. N + 3, pair offsets, bumps 0.001 .. 0.5, r = 0 among the rates.  Whatever the seed,
    the first eight deal both storages, both column widths of the sweep (stored columns even or odd), GBM and Heston schemes
    0, 1, 3, a chain of one entry, one of more than 16 (two groups) and r = 0."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        j = i % 8
        model = ("gbm", "gbm", "heston", "gbm", "heston", "gbm", "heston", "gbm")[j]
        folded = model == "gbm" and j in (0, 3, 7)
        # pairs even or odd: folded storage keeps one column per pair, so an odd count takes the one-column sweep
        M = 2 * (int(rng.integers(600, 1500)) * 2 + (1 if j in (1, 3, 4) else 0))
        N = int(rng.integers(1, 71))
        ne = 1 if j == 2 else (int(rng.integers(17, 21)) if j == 5 else int(rng.integers(1, 21)))
        S0 = float(rng.uniform(40.0, 160.0))
        cases.append(dict(
            M=M, N=N, model=model, folded=folded, scheme=(0, 1, 3)[(i // 2) % 3] if model == "heston" else 0, S0=S0,
            strikes=[float(S0 * rng.uniform(0.7, 1.3)) for _ in range(ne)], puts=[bool(rng.integers(0, 2)) for _ in range(ne)],
            every=[int(rng.integers(0, N + 4)) for _ in range(ne)],
            r=0.0 if j == 6 else float(rng.uniform(0.01, 0.08)), sigma=float(rng.uniform(0.15, 0.5)),
            T=float(rng.uniform(0.25, 2.0)), bump=float(math.exp(rng.uniform(math.log(0.001), math.log(0.5)))),
            seed=int(rng.integers(1, 2 ** 31)), stream=int(rng.integers(0, 8)),
            pair_offset=int(rng.integers(0, 2 ** 20)) if i % 2 else 0))
    return cases

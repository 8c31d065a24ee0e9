"""numpy restatement of the multi-policy inner sweep of the chain price bounds (chain_bounds_inner_body,
omc_chain_bounds_dev.h): E frozen policies on ONE simulation of every inner pair.  TEST INFRASTRUCTURE
ONLY.

The spots are the caller's -- inner(i, t) -> [N - t + 1][n_inner] float32 in the antithetic layout of helpers/bounds_ref.py
(column j and column j + n_inner/2 are the partners of pair j; row 0 = S_t[i]) -- and shared by all entries.  The sweep walks
an item's pairs date by date WHILE SOME ENTRY HAS A LIVE PARTNER, as the kernel does: per entry the first date its rule fires
(bounds_ref.stop_rule on the entry's own K, side and table; the expiry stops everyone), the index there, and at the end the
pair value bd_value(a) + bd_value(b) = D[tau_a] max(phi(x_a), 0) + D[tau_b] max(phi(x_b), 0).  Per entry: Q^ and the integer
sum of (tau_a - t) + (tau_b - t), the single call's inner_path_steps.  For the chain: the steps simulated, per partner the
LARGEST stop date over the entries.
"""
from __future__ import annotations

import numpy as np

from helpers import bounds_ref as br


def item(S, t, N, r, T, entries):
    """One item's shared inner paths S [N - t + 1][2 H] against the entries [(K, is_put, betas4)] -> dict q [E] (the means),
    steps [E] (ints), simulated (int), swept (the dates the sweep visited), ties."""
    E, m = len(entries), S.shape[1]
    H = m // 2
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    tau = np.zeros((E, m), np.int64)  # 0 while live, as the kernel's stop dates
    x = np.zeros((E, m), np.float32)
    ties = 0
    k = 0
    while (tau == 0).any():  # every entry stops at d = N, so k never passes N - t
        k += 1
        d = t + k
        assert d <= N
        for e, (K, is_put, b4) in enumerate(entries):
            st, ti = br.stop_rule(S[k], d, N, K, is_put, b4)
            ties += ti if d < N else 0
            ex = (tau[e] == 0) & st
            tau[e][ex] = d
            x[e][ex] = S[k][ex]
    q = np.zeros(E)
    steps = []
    for e, (K, is_put, _) in enumerate(entries):
        xd = x[e].astype(np.float64)
        Z = D[tau[e]] * np.maximum((K - xd) if is_put else (xd - K), 0.0)
        q[e] = (Z[:H] + Z[H:]).sum() / (2 * H)  # per pair bd_value(a) + bd_value(b)
        steps.append(int((tau[e] - t).sum()))
    return dict(q=q, steps=steps, simulated=int((tau.max(axis=0) - t).sum()), swept=k, ties=ties)


def q_rows(So, inner, rows, r, T, entries):
    """Q^_t[i] of every entry for the outer paths i in `rows`, all dates -> dict q [E][len(rows)][N], inner_path_steps [E],
    simulated, ties"""
    N = So.shape[0] - 1
    E = len(entries)
    q = np.zeros((E, len(rows), N))
    steps, sim, ties = [0] * E, 0, 0
    for k, i in enumerate(rows):
        for t in range(N):
            it = item(inner(i, t), t, N, r, T, entries)
            q[:, k, t] = it["q"]
            steps = [a + b for a, b in zip(steps, it["steps"])]
            sim += it["simulated"]
            ties += it["ties"]
    return dict(q=q, inner_path_steps=steps, simulated=sim, ties=ties)


def numpy_gbm_case(seed, N=5, n_outer=4, n_inner=8, S0=100.0, r=0.05, sigma=0.3, T=1.0):
    """a tiny set of outer and inner GBM paths from numpy's generator (float32 spots, antithetic layout): So [N+1][n_outer]
    and inner(i, t)"""
    rng = np.random.default_rng(seed)
    dt = T / N
    a, b = (r - 0.5 * sigma * sigma) * dt, sigma * np.sqrt(dt)

    def paths(s0, z):  # z [steps][H] -> [steps + 1][2 H]
        zz = np.concatenate([z, -z], axis=1)
        out = np.empty((z.shape[0] + 1, zz.shape[1]), np.float32)
        out[0] = s0
        for k in range(z.shape[0]):
            out[k + 1] = (out[k].astype(np.float64) * np.exp(a + b * zz[k])).astype(np.float32)
        return out

    So = paths(np.float32(S0), rng.standard_normal((N, n_outer // 2)))
    Z = rng.standard_normal((n_outer, N, N, n_inner // 2))
    return So, lambda i, t: paths(So[t, i], Z[i, t][:N - t])

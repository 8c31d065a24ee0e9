"""numpy restatement of the Andersen-Broadie price bounds for barrier options (omc_price_american_bounds_barrier; the
definitions are in DESIGN.md section 31 and include/omc_barrier_bounds.h), built on tests/helpers/bounds_ref.py,
bounds_schedule_ref.py, bounds_check_ref.py and barrier_ref.py.  TEST INFRASTRUCTURE ONLY.

A path is a column of REAL float32 spots with a hit step (barrier_ref.discrete_hit_steps: the first row whose float64
spot passes H, rows + 1 = never; 0 = hit before row 0, a restart).  What the policy sees is the ENCODED index
(barrier_ref.encode): the spot where the option is live, the dead spot elsewhere -- a knock-out is dead at its hit row and
after it, a knock-in is live from its hit row on.
The game is bounds_ref's on the encoded index with one more reason to stop: a knocked-out path stops, with the value of the
dead index (0), at the first exercise date at or after its hit row.  An item (i, t) of a knock-out that is dead at t is not
simulated: Q^ = 0.0 and no steps.  Which walk the device runs is restated too: the list-driven walk over the kept dates for a
knock-out and for the payoff check, the dense walk for a knock-in, the scheduled walk with a schedule.
"""
from __future__ import annotations

import math

import numpy as np

from helpers import barrier_ref as bar
from helpers import bounds_check_ref as bcr
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bsr

KINDS = bar.KINDS


def knock_out(kind):
    return kind.endswith("-out")


def first_hit(S, kind, H):
    """the device's hit array: the first step 1 .. N at which the column is hit, 0 = never (int32)"""
    N = S.shape[0] - 1
    hs = bar.discrete_hit_steps(S, kind, H)
    return np.where(hs > N, 0, hs).astype(np.int32)


def local_hits(S, kind, H, start_hit=False):
    """hit rows of the columns of S [n+1][m] counted from row 0: 0 with start_hit, n + 1 = never"""
    if start_hit:
        return np.zeros(S.shape[1], np.int64)
    return bar.discrete_hit_steps(S, kind, H)


def encode(S, kind, H, K, is_put, start_hit=False):
    """-> (encoded index [n+1][m] float32, hit rows [m])"""
    hs = local_hits(S, kind, H, start_hit)
    return bar.encode(S, kind, H, hs, K, is_put), hs


def first_stop(E, hs, kind, t0, N, K, r, T, is_put, betas4, k=0):
    """bounds_ref.first_stop on the encoded rows E [N - t0 + 1][m] (row j = date t0 + j) with the knock-out stop: at the
    exercise dates (every date; with k >= 2 the scheduled ones) a live path stops where the rule fires on its index or where
    it is knocked out (hs <= j) -> (tau, Z, ties)"""
    m = E.shape[1]
    bk = bsr.mask(betas4, k)
    dates = set(bsr.schedule(N, k)[1:])
    ko = knock_out(kind)
    tau = np.full(m, -1, np.int64)
    x = np.zeros(m, np.float32)
    ties = 0
    for j in range(1, N - t0 + 1):
        d = t0 + j
        if d not in dates:
            continue
        st, ti = br.stop_rule(E[j], d, N, K, is_put, bk)
        if ko:
            st = st | (hs <= j)
        ties += ti if d < N else 0
        ex = (tau < 0) & st
        tau[ex] = d
        x[ex] = E[j][ex]
    phi = (K - x.astype(np.float64)) if is_put else (x.astype(np.float64) - K)
    D = np.exp(-r * (T / N) * np.arange(N + 1))
    return tau, D[tau] * np.maximum(phi, 0.0), ties


def lower_bound(S, kind, H, K, r, T, is_put, betas4, k=0):
    """S: the REAL lower-bound paths [N+1][n_lower] (antithetic layout) -> bounds_ref.lower_bound's dict"""
    N = S.shape[0] - 1
    E, hs = encode(S, kind, H, K, is_put)
    tau, Z, ties = first_stop(E, hs, kind, 0, N, K, r, T, is_put, betas4, k)
    lo, se, ratio = br._pair_mean_se(Z)
    return dict(lower=lo, se_lower=se, se_cancel=ratio, n_exercised=int(np.count_nonzero(tau < N)), ties=ties)


def dead_items(hit, N, kind):
    """[N][n_outer] bool: item (i, t) of a knock-out is dead at its start (a knock-in has no such item)"""
    hit = np.asarray(hit)
    t = np.arange(N)[:, None]
    return (hit[None, :] != 0) & (hit[None, :] <= t) & knock_out(kind)


def upper_bound(So, inner, kind, H, K, r, T, is_put, betas4, k=0, check=None):
    """So: the REAL outer paths [N+1][n_outer]; inner(i, t) -> the REAL inner paths of item (i, t) [N - t + 1][n_inner] (row 0 =
    So[t, i]).  k >= 2: the scheduled game; check "payoff": the payoff check (never both) -> dict upper, se_upper, q, samples,
    keep [N][n_outer], hit, Eo, inner_path_steps, ties, zmax"""
    N, n = So.shape[0] - 1, So.shape[1]
    assert not (int(k) >= 2 and check)
    Eo, _ = encode(So, kind, H, K, is_put)
    hit = first_hit(So, kind, H)
    dead = dead_items(hit, N, kind)
    ties = 0
    if check == "payoff":
        kd = bcr.keep(Eo, betas4, 1, K, r, T, is_put)
        kp, ties = kd["keep"], kd["ties"]
        assert not (kp & dead).any()  # the payoff check drops every dead item by construction
    else:
        kp = ~dead
    ts = bsr.schedule(N, k)[:-1] if int(k) >= 2 else range(N)
    q = np.zeros((n, N))
    steps = 0
    for i in range(n):
        for t in ts:
            if not kp[t, i]:
                continue
            started_hit = bool(hit[i] != 0 and hit[i] <= t)
            E, hs = encode(inner(i, t), kind, H, K, is_put, start_hit=started_hit)
            tau, Z, ti = first_stop(E, hs, kind, t, N, K, r, T, is_put, betas4, k)
            q[i, t] = Z.sum() / Z.size
            steps += int((tau - t).sum())
            ties += ti
    rows = range(n)
    if int(k) >= 2:
        wk = bsr.walk_rows(Eo, q, rows, K, r, T, is_put, betas4, k)
    elif check == "payoff" or knock_out(kind):
        wk = bcr.walk_rows(Eo, q, rows, kp, K, r, T, is_put, betas4)
    else:
        wk = br.walk_rows(Eo, q, rows, K, r, T, is_put, betas4)
    up, se, ratio = br._pair_mean_se(wk["samples"])
    return dict(upper=up, se_upper=se, se_cancel=ratio, q=q, samples=wk["samples"], keep=kp, hit=hit, Eo=Eo,
                inner_path_steps=steps, ties=ties + wk["ties"], zmax=wk["zmax"])


def check_against_restatement(p, dev, sp, kind, H, k, check, n_lower, n_outer, n_inner, rtol=1e-12):
    """The device's result dict `dev` (want_q, want_samples) against the restatement on the device's own REAL spots `sp` (Sl,
    So, inner): no ties, equal counts, q / samples / bounds at rtol (atol rtol K, as tests/test_gpu_bounds.py) -> (lo, up)"""
    K, is_put = float(p.K), bool(p.is_put)
    lo = lower_bound(sp["Sl"], kind, H, K, p.r, p.T, is_put, dev["betas"], k)
    up = upper_bound(sp["So"], sp["inner"], kind, H, K, p.r, p.T, is_put, dev["betas"], k, check)
    assert lo["ties"] == 0 and up["ties"] == 0  # numpy's decisions are the device's
    assert dev["n_exercised_lower"] == lo["n_exercised"]
    assert dev["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(dev["q"], up["q"], rtol=rtol, atol=rtol * K)
    np.testing.assert_allclose(dev["samples"], up["samples"], rtol=rtol, atol=rtol * K)
    for key in ("lower", "se_lower"):
        np.testing.assert_allclose(dev[key], lo[key], rtol=rtol, atol=rtol * K, err_msg=key)
    for key in ("upper", "se_upper"):
        np.testing.assert_allclose(dev[key], up[key], rtol=rtol, atol=rtol * K, err_msg=key)
    assert dev["ci_lo"] == dev["lower"] - 1.96 * dev["se_lower"] and dev["ci_hi"] == dev["upper"] + 1.96 * dev["se_upper"]
    assert (dev["n_lower"], dev["n_outer"], dev["n_inner"]) == (n_lower, n_outer, n_inner)
    return lo, up


def never_exercise_table(N):
    """policy `given` with n = 0 on every date: a path stops at N (or where it is knocked out)"""
    return np.zeros((N + 1, 4))


def european(S, kind, H, K, r, T, is_put):
    """the discounted payoff mean of the European option of `kind` on the REAL paths S (omc_price_barrier's euro_out /
    euro_in: float64 payoffs of the float32 terminal spot, summed exactly)"""
    N = S.shape[0] - 1
    hit = bar.discrete_hit_steps(S, kind, H) <= N
    x = S[N].astype(np.float64)
    pay = np.maximum(K - x if is_put else x - K, 0.0) * math.exp(-r * T)
    v = np.where(hit, pay, 0.0) if kind.endswith("-in") else np.where(hit, 0.0, pay)
    return math.fsum(v) / v.size

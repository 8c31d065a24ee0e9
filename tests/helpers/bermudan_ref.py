"""Bermudan exercise schedules of the option chain (omc_chain_entry::exercise_every), restated.

An entry with exercise_every = k >= 2 may exercise early only at the dates t in 1 .. N-1 with (N - t) % k == 0.  Its value
is the two-pass flow with every other date skipped in both passes:

  full storage     the C oracle: the two-pass fits of orc_lsm_poly, then orc_lsm_apply_frozen with nitm[t] = 0 at every
                   unscheduled date (`masked_replay`)
  folded storage   `folded_two_pass`: a float64 restatement of orc_lsm_two_pass_folded with a date mask, from the first
                   partners alone -- the partner of a stored spot enters through u' = cK[t] / S_t - 1, cK from the
                   oracle's fold_constants / fold_table
  `matrix_two_pass` the same flow on an explicit float64 matrix (the partner matrix C_t / S_t written out): what the folded
                   restatement must be consistent with

Every restatement reports `margin`: the smallest |immediate - continuation| / K over the decisions it took.  A decision
within 1e-10 of a tie is the one thing two correct implementations may decide differently (tests/test_gpu_fuzz.py)."""
import math

import numpy as np

from oracle import cpu as orc

TIE = 1e-10


def schedule(N, k):
    """bool [N+1]: True at the early-exercise dates of exercise_every = k on a grid of N dates."""
    m = np.zeros(N + 1, bool)
    for t in range(1, N):
        m[t] = k < 2 or (N - t) % k == 0
    return m


def n_early(N, k):
    return int(schedule(N, k).sum())


# ------------------------------------------------------------------ full storage: the oracle's masked replay
def masked_replay(S, K, r, T, is_put, k):
    """orc_lsm_apply_frozen with the two-pass fits and nitm[t] = 0 off the schedule -> the oracle's dict plus sum_nitm,
    nitm (masked), betas4 [N+1][4] (b0, b1, b2, n; zero rows off the schedule) and margin."""
    S = np.ascontiguousarray(S, np.float32)
    N = S.shape[0] - 1
    two = orc.lsm_poly(S, K, r, T, is_put, "two_pass")
    mask = schedule(N, k)
    nitm = np.where(mask, two["nitm"], 0).astype(np.int64)
    out = orc.lsm_apply_frozen(S, K, r, T, is_put, two["betas"], nitm)
    betas4 = np.zeros((N + 1, 4))
    betas4[mask, :3] = two["betas"][mask]
    betas4[mask, 3] = two["nitm"][mask]
    out.update(sum_nitm=int(nitm.sum()), nitm=nitm, betas4=betas4, n_paths=S.shape[1],
               margin=_replay_margin(S, K, is_put, two["betas"], nitm))
    return out


def _replay_margin(S, K, is_put, betas, nitm):
    """min |imm - cont| / K over the in-the-money spots of every decided date (alive or not: a superset of the decisions)"""
    best = math.inf
    for t in np.nonzero(nitm)[0]:
        s = S[t].astype(np.float64)
        imm = (K - s) if is_put else (s - K)
        u = s / K - 1.0
        cont = u * (u * betas[t, 2] + betas[t, 1]) + betas[t, 0]
        itm = imm > 0.0
        if itm.any():
            best = min(best, float(np.abs(imm - cont)[itm].min()) / K)
    return best


# ------------------------------------------------------------------ the flow on (moneyness, payoff) rows, float64
def _flow(U, PAY, r, T, K, mask):
    """U, PAY: [N+1][paths] moneyness and payoff of every path at every date.  Pass 1 regresses the discounted terminal
    payoff on [1, u, u^2] over the in-the-money rows of every scheduled date (the oracle's solver on the eight sums);
    pass 2 is the sticky backward rule over the scheduled dates that have a regression set; valued at exp(-r dt (tex - 1))."""
    N = U.shape[0] - 1
    dt = T / N
    D = np.exp(-r * dt * np.arange(N + 1, dtype=np.float64))
    pN = np.where(PAY[N] > 0.0, PAY[N], 0.0)
    mom = np.zeros((N + 1, 8))
    for t in range(1, N):
        if not mask[t]:
            continue
        itm = PAY[t] > 0.0
        u, y = U[t][itm], pN[itm] * D[N - t]
        u2 = u * u
        mom[t] = [u.size, u.sum(), u2.sum(), (u2 * u).sum(), (u2 * u2).sum(), y.sum(), (u * y).sum(), (u2 * y).sum()]
    betas4 = orc.solve_poly2(mom)
    betas4[~mask] = 0.0
    betas4[0] = betas4[N] = 0.0
    nitm = mom[:, 0].astype(np.int64)
    tex = np.full(U.shape[1], N, np.int32)
    pay = PAY[N].copy()
    margin = math.inf
    for t in range(N - 1, 0, -1):
        if not mask[t] or nitm[t] == 0:
            continue
        b = betas4[t]
        cont = U[t] * (U[t] * b[2] + b[1]) + b[0]
        can = (tex == N) & (PAY[t] > 0.0)
        if can.any():
            margin = min(margin, float(np.abs(PAY[t] - cont)[can].min()) / K)
        ex = can & (PAY[t] > cont)
        tex[ex] = t
        pay[ex] = PAY[t][ex]
    cf = np.where(pay > 0.0, pay, 0.0) * D[tex - 1]
    return dict(price=float(cf.sum()) / cf.size, sum=float(cf.sum()), sumsq=float((cf * cf).sum()), n_paths=int(cf.size),
                n_exercised=int((tex < N).sum()), n_zero=int((cf == 0.0).sum()), sum_nitm=int(nitm[1:N].sum()),
                betas4=betas4, nitm=nitm, tex=tex, margin=margin)


def folded_two_pass(S_half, K, r, T, is_put, c0, g, k=1, cK=None):
    """The two-pass flow over BOTH partners of every pair from the first partners S_half [N+1][P] alone, dates off the
    schedule of k skipped.  -> _flow's dict with texa / texb (the stored paths' and the partners' exercise dates).
    cK: the fold table to use instead of the oracle's fold_table(N, c0, g) (rows of a longer grid's table)."""
    S = np.ascontiguousarray(S_half, np.float32).astype(np.float64)
    N, P = S.shape[0] - 1, S.shape[1]
    cK = orc.fold_table(N, c0, g) if cK is None else np.asarray(cK, np.float64)
    ua = S * (1.0 / K) - 1.0
    pa = (K - S) if is_put else (S - K)
    ub = cK[:, None] * (1.0 / S) - 1.0
    pb = (-K * ub) if is_put else (K * ub)
    out = _flow(np.concatenate([ua, ub], axis=1), np.concatenate([pa, pb], axis=1), r, T, K, schedule(N, k))
    out["texa"], out["texb"] = out["tex"][:P], out["tex"][P:]
    return out


def partner_matrix(S_half, K, c0, g):
    """[S | C_t / S] in float64: the matrix whose second half are the partners the folded sweeps never store."""
    S = np.ascontiguousarray(S_half, np.float32).astype(np.float64)
    cK = orc.fold_table(S.shape[0] - 1, c0, g)
    return np.concatenate([S, cK[:, None] * K / S], axis=1)


def matrix_two_pass(S64, K, r, T, is_put, k=1):
    """The masked two-pass flow on an explicit float64 matrix."""
    S = np.asarray(S64, np.float64)
    return _flow(S * (1.0 / K) - 1.0, (K - S) if is_put else (S - K), r, T, K, schedule(S.shape[0] - 1, k))


# ------------------------------------------------------------------ comparisons
def agrees(dev, ref, rel=1e-9):
    """The comparison of the American pricings with their oracles (tests/test_gpu_fold.py, test_gpu_dividends.py): counts
    equal, price / sum / sumsq within rel.  -> (ok, what differs)"""
    bad = [k for k in ("n_exercised", "n_zero", "sum_nitm") if int(dev[k]) != int(ref[k])]
    for k in ("price", "sum", "sumsq"):
        if not abs(dev[k] - ref[k]) <= rel * abs(ref[k]) + 1e-300:
            bad.append(k)
    return not bad, bad


def assert_agrees(dev, ref, what=""):
    """agrees, or the reference took a decision within TIE of a tie (then the two may differ by that decision)."""
    ok, bad = agrees(dev, ref)
    show = {k: (dev[k], ref[k]) for k in ("price", "sum", "sumsq", "n_exercised", "n_zero", "sum_nitm")}
    print(what, "margin", ref["margin"], show)
    assert ok or ref["margin"] <= TIE, (what, bad, ref["margin"], show)


# ------------------------------------------------------------------ seeded cases of tests/test_gpu_bermudan_fuzz.py
HESTON = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)


def fuzz_cases(n, seed):
    """Random (N in 1 .. 70, k, ragged M, storage, model, pair offset).  Whatever the seed, the first eight deal both
    storages, both load widths (columns a multiple of four or not), GBM and Heston schemes 0, 1, 3, N % k != 0, k >= N
    (no early date) and a schedule of one date."""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        j = i % 8
        model = ("gbm", "gbm", "heston", "gbm", "heston", "gbm", "heston", "gbm")[j]
        folded = model == "gbm" and j in (0, 3, 7)
        # columns a multiple of four (16-byte loads; folded: of eight, the stored half counts), or 4 x + 2 (scalar loads)
        M = int(rng.integers(300, 1500)) * 8 if j % 2 == 0 else int(rng.integers(600, 3000)) * 4 + 2
        N = int(rng.integers(1, 71))
        if j == 1:
            N = int(rng.integers(8, 71))
            k = int(rng.integers(3, N))
            while N % k == 0:
                k += 1
        elif j == 3:
            k = N + int(rng.integers(0, 4))        # no early date
        elif j == 5:
            N = int(rng.integers(5, 71))
            k = N - 1                              # one early date: t = 1
        else:
            k = int(rng.integers(2, max(3, N + 2)))
        k = max(k, 2)
        S0 = float(rng.uniform(40.0, 160.0))
        cases.append(dict(M=M, N=N, k=k, model=model, folded=folded, scheme=(0, 1, 3)[(i // 2) % 3] if model == "heston" else 0,
                          S0=S0, K=float(S0 * rng.uniform(0.85, 1.15)), r=float(rng.uniform(0.01, 0.08)),
                          sigma=float(rng.uniform(0.15, 0.5)), T=float(rng.uniform(0.25, 2.0)), is_put=bool(rng.integers(0, 2)),
                          seed=int(rng.integers(1, 2 ** 31)), stream=int(rng.integers(0, 8)),
                          pair_offset=int(rng.integers(0, 2 ** 20)) if i % 2 else 0))
    return cases


def oracle_paths(c, half=False):
    """The C oracle's paths of a fuzz case (full matrix; half: the first partners of a folded GBM case)."""
    if c["model"] == "gbm":
        if half:
            return orc.gbm_paths(c["M"] // 2, c["N"], c["S0"], c["r"], c["sigma"], c["T"], c["seed"], c["stream"],
                                 c["pair_offset"], antithetic=0)
        return orc.gbm_paths(c["M"], c["N"], c["S0"], c["r"], c["sigma"], c["T"], c["seed"], c["stream"], c["pair_offset"])
    h = HESTON
    return orc.heston_paths(c["M"], c["N"], c["S0"], c["r"], c["T"], h["v0"], h["kappa"], h["theta"], h["xi"], h["rho"],
                            c["seed"], c["stream"], c["pair_offset"], c["scheme"])


def reference(c, S):
    """The restatement of a case on the matrix S (folded: the first partners)."""
    if c["folded"]:
        c0, g = orc.fold_constants(c["S0"], c["K"], c["r"], c["sigma"], c["T"], c["N"])
        return folded_two_pass(S, c["K"], c["r"], c["T"], c["is_put"], c0, g, c["k"])
    return masked_replay(S, c["K"], c["r"], c["T"], c["is_put"], c["k"])

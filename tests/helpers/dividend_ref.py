"""numpy restatement of the dividend semantics (include/omc.h).  TEST INFRASTRUCTURE ONLY.

schedule()  the per-step table of a dividend schedule, to float32 bits (what omc_dividend_schedule returns)
apply()     the path matrix with dividends from a VANILLA matrix at drift r - q, whatever the model: the vanilla
            generator's own growth factors V_t / V_{t-1}, re-applied in float64 to the spot that has paid its dividends.
            Each ratio of two float32 spots carries up to 2^-23 of rounding, so N steps are good to about N * 1.2e-7: the
            tests that compare the device with it keep N <= 64 (7.6e-6, under half the path tolerance of DESIGN.md
            section 4: 2e-5 GBM, 5e-5 Heston) and take atol = rtol * the column's largest vanilla spot, since a cash
            dividend can take a spot close to 0, where a relative bound on the result would ask for more digits than the
            vanilla spots have.
bsm()       the Black-Scholes-Merton closed form with a continuous yield.
"""
import math

import numpy as np

KINDS = {"proportional": 0, "cash": 1}


def ex_step(t, T, n_steps):
    return min(max(int(math.ceil(t * n_steps / T - 1e-9)), 1), n_steps)


def _norm(dividends):
    out = []
    for d in dividends:
        kind = d[2] if len(d) == 3 else "cash"
        out.append((float(d[0]), float(d[1]), KINDS[kind] if isinstance(kind, str) else int(kind)))
    return out


def schedule(T, n_steps, dividends):
    """-> (mul float32 [N+1], cash float32 [N+1], has bool [N+1])"""
    divs = _norm(dividends)
    steps = [ex_step(t, T, n_steps) for t, _, _ in divs]
    order = sorted(range(len(divs)), key=lambda i: steps[i])  # stable: input order within a step
    m = np.ones(n_steps + 1, np.float64)
    c = np.zeros(n_steps + 1, np.float64)
    has = np.zeros(n_steps + 1, bool)
    for i in order:
        k, (_, amount, kind) = steps[i], divs[i]
        if kind == 0:
            m[k] *= 1.0 - amount
            c[k] *= 1.0 - amount
        else:
            c[k] += amount
        has[k] = True
    return m.astype(np.float32), c.astype(np.float32), has


def apply(V, mul, cash, has):
    """V [N+1][M] vanilla spots at drift r - q -> float64 [N+1][M] with the dividends of the table applied"""
    V = np.asarray(V, np.float64)
    out = np.empty_like(V)
    out[0] = V[0]
    for t in range(1, V.shape[0]):
        with np.errstate(invalid="ignore", divide="ignore"):
            s = out[t - 1] * (V[t] / V[t - 1])
        if has[t]:
            s = np.maximum(s * np.float64(mul[t]) - np.float64(cash[t]), 0.0)
        out[t] = s
    return out


def tolerance(V, rtol):
    """atol per column for a comparison with apply(V, ..): rtol * the column's largest vanilla spot"""
    return rtol * np.abs(np.asarray(V, np.float64)).max(axis=0)


def close(S, ref, V, rtol):
    """|S - ref| <= rtol |ref| + tolerance(V, rtol), element-wise -> (ok, worst excess ratio)"""
    err = np.abs(np.asarray(S, np.float64) - ref)
    bound = rtol * np.abs(ref) + tolerance(V, rtol)[None, :]
    return bool(np.all(err <= bound)), float((err / bound).max())


def _ncdf(x):
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def bsm(S, K, r, q, sigma, T, is_put):
    d1 = (math.log(S / K) + (r - q + 0.5 * sigma * sigma) * T) / (sigma * math.sqrt(T))
    d2 = d1 - sigma * math.sqrt(T)
    if is_put:
        return K * math.exp(-r * T) * _ncdf(-d2) - S * math.exp(-q * T) * _ncdf(-d1)
    return S * math.exp(-q * T) * _ncdf(d1) - K * math.exp(-r * T) * _ncdf(d2)

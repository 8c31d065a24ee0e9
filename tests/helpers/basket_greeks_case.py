"""What the multi-asset Greeks tests share (omc_price_american_basket_greeks).  TEST INFRASTRUCTURE ONLY.

reference()  the numpy restatement (tests/helpers/basket_greeks_ref.py) on the DEVICE's own matrices: S_keep and assets_keep
             of an omc_price_american_basket call at the same parameters, with the policy the Greeks call returned
agrees()     the comparison, in the manner of tests/helpers/greeks_check.agrees: exercise counts of every chain identical --
             unless the restatement shows at least as many decisions of that chain family within 1e-10 K of the
             continuation value -- and every value to rel 1e-9 / abs 1e-12, standard errors to rel 1e-6
fuzz_cases() the seeded cases of tests/test_gpu_basket_greeks_fuzz.py; needs no GPU (tests/test_basket_greeks_cpu.py)
"""
from __future__ import annotations

import math

import numpy as np

from helpers import basket_greeks_ref as bgr
from helpers.basket_bounds_case import index_and_assets, random_correlation, with_fields  # noqa: F401
from helpers.greeks_check import close
from options_model_amd import _ffi

KINDS = ("basket", "geometric", "best-of", "worst-of")
PER_ASSET = ("delta", "vega", "gamma", "price_up", "price_down")


def law_of(b):
    """the per-asset arguments of a Basket, as the restatement takes them"""
    d = int(b.n_assets)
    return dict(S0=list(b.S0)[:d], sigma=list(b.sigma)[:d], q=list(b.q)[:d], w=list(b.w)[:d], kind=int(b.kind))


def reference(ctx, p, b, betas, h, gamma=True):
    S, A = index_and_assets(ctx, p, b)
    return bgr.greeks(A, S, float(p.K), float(p.r), float(p.T), bool(p.is_put), betas, h=h, gamma=gamma, **law_of(b))


def agrees(dev, ref, d, gamma=True):
    """Asserts the agreement above -> True when the values were compared, False when a tie went the other way (the counts
    differ by no more than the restatement's ties, and the values then move by those paths' share: not compared)."""
    diff = [abs(dev["n_exercised"] - ref["n_exercised"]), 0, 0]
    if gamma:
        diff[1] = sum(abs(a - r) for a, r in zip(dev["n_exercised_up"], ref["n_exercised_up"]))
        diff[2] = sum(abs(a - r) for a, r in zip(dev["n_exercised_down"], ref["n_exercised_down"]))
    for df, ties in zip(diff, ref["ties"]):
        assert df <= ties, (diff, ref["ties"])
    if any(diff):
        return False
    assert dev["n_zero"] == ref["n_zero"]
    for k in ("price", "rho", "theta"):
        assert close(dev[k], ref[k]), (k, dev[k], ref[k])
    for k in ("rho", "theta"):
        assert close(dev["se_" + k], ref["se_" + k], rel=1e-6), (k, dev["se_" + k], ref["se_" + k])
    for k in PER_ASSET:
        if not gamma and k in ("gamma", "price_up", "price_down"):
            assert all(math.isnan(x) for x in dev[k]), k
            continue
        assert len(dev[k]) == len(ref[k]) == d
        for i in range(d):
            assert close(dev[k][i], ref[k][i]), (k, i, dev[k][i], ref[k][i])
            if not k.startswith("price"):
                assert close(dev["se_" + k][i], ref["se_" + k][i], rel=1e-6), (k, i, dev["se_" + k][i], ref["se_" + k][i])
    return True


def strip(d):
    """a result dict without what legitimately differs between identical calls"""
    return {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in d.items() if not k.startswith("ms_") and k != "timed"}


def nan_equal(a, b):
    """dict equality where NaN equals NaN (the gamma fields of a call without gamma)"""
    def norm(v):
        if isinstance(v, list):
            return [norm(x) for x in v]
        return "nan" if isinstance(v, float) and math.isnan(v) else v
    return {k: norm(v) for k, v in a.items()} == {k: norm(v) for k, v in b.items()}


# ---------------------------------------------------------------------------------------------- the fuzz cases
def fuzz_cases(n, seed=20261018):
    """n seeded cases, as plain dicts: d in 1 .. 8 and the four kinds (both cycled), N in 1 .. 70, an odd pair count, a
    pair offset, a bump in 0.001 .. 0.5 (log-uniform), r = 0 on every fifth, put / call, every third with a given table
    with n = 0 holes, every fourth without gamma."""
    rng = np.random.default_rng(seed)
    perm_d = rng.permutation(8)
    out = []
    for c in range(n):
        d = int(perm_d[c % 8]) + 1
        kind = KINDS[(c + c // 4) % 4]
        N = int(rng.integers(1, 71)) if c % 6 else (1, 2)[(c // 6) % 2]
        case = dict(d=d, kind=kind, N=N, M=2 * (2 * int(rng.integers(150, 900)) + 1), is_put=bool(rng.integers(0, 2)),
                    given=c % 3 == 2, gamma=c % 4 != 3, bump=float(10.0 ** rng.uniform(-3.0, math.log10(0.5))),
                    r=0.0 if c % 5 == 4 else float(rng.uniform(0.01, 0.08)), seed=int(rng.integers(1, 1 << 31)),
                    stream=int(rng.integers(0, 50)), pair_offset=int(rng.integers(0, 1 << 36)),
                    S0=[float(x) for x in rng.uniform(85.0, 115.0, d)], sigma=[float(x) for x in rng.uniform(0.1, 0.4, d)],
                    q=[float(x) for x in rng.uniform(0.0, 0.08, d)], rho=random_correlation(rng, d), T=float(rng.uniform(0.5, 3.0)))
        w = rng.uniform(0.5, 1.5, d)
        case["w"] = [float(x) for x in (w / w.sum() if kind in ("basket", "geometric") else w / w.mean())]
        case["holes"] = [bool(x) for x in rng.random(N + 1) < 0.3]
        out.append(case)
    return out


def fuzz_params(case):
    p = _ffi.make_params(model="gbm", is_put=case["is_put"], semantics="two_pass", n_paths=case["M"], n_steps=case["N"],
                         S0=case["S0"][0], K=100.0, r=case["r"], sigma=case["sigma"][0], T=case["T"], seed=case["seed"],
                         stream=case["stream"], pair_offset=case["pair_offset"])
    b = _ffi.make_basket(case["S0"], case["sigma"], case["q"], case["w"], case["rho"], case["kind"])
    return p, b


def given_table(ctx, p, b, holes):
    """a policy from other paths (stream 9 of p's seed): the fits of a Greeks call there, with n = 0 on the dates `holes` marks"""
    t = ctx.price_american_basket_greeks(with_fields(p, n_paths=2048, stream=9, pair_offset=0), b, gamma=False,
                                         want_betas=True)["betas"].copy()
    t[np.asarray(holes), 3] = 0.0
    return t

"""omc_price_american_div_greeks (include/omc_dividend_greeks.h) on the GPU, against the numpy
restatement (helpers/dividend_greeks_ref.py) on the device's OWN matrices -- omc_price_american_div's S_keep at S0,
S0 (1 + h) and S0 (1 - h) -- and the generator's own normals.

  1. the scenario paths are the generator's: with a policy that stops every in-the-money path at a chosen step, price,
     price_up and price_down equal the restatement's to the order of the float64 sum (1e-9), every count exactly
  2. the base pricing: counts and sum_nitm of omc_price_american_div, price 1e-9, betas_out the bits of omc_lsm_poly's fits
  3. the Greeks against the restatement, every schedule of the list, GBM and Heston schemes 0, 1 and 3, put and call
  4. no dividends, q = 0: every Greek of omc_price_american_greeks on full storage
  5. a cash dividend of amount 0 changes no bit
  6. the European policy with proportional dividends and a yield: the Black-Scholes-Merton closed form within 4 se
  7. the floor: floored and live paths together; a schedule that floors every path gives delta = gamma = 0 exactly
  8. identical calls return identical bits; the call's own betas_out as betas returns the same Greeks
  9. the C error codes

TOL is MEASURED: the worst relative error of each Greek over 1, 3, 4, 6 and the fuzz sweep (DESIGN.md 32.4 lists them), times 4.
The sweep carries float32 spots and tangents through N steps; the restatement reads the float32 matrix and steps float64
tangents, so per path the two differ by float32 rounding of the tangents, some 1e-7, and the means by far less.  CAP keeps
every tolerance below 1 % of the Greek's own standard error (the smallest se / |Greek| met is 1.8e-3: rho): a tolerance near the
Monte-Carlo error would hide a wrong term.
Shapes: n_paths 2 (3 * 256 + 5) (a ragged last workgroup) and 4096, n_steps 5, 7, 12 (odd for Heston's two steps per Philox
block, no multiple of 4 for GBM's four)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import call_catalogue as cat
from helpers import dividend_bounds_case as dc
from helpers import dividend_greeks_case as gc
from helpers import dividend_greeks_ref as gr
from helpers import dividend_ref as dr
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

# 4 x the worst measured relative error over the 74 comparisons of this file and the fuzz sweep at scale 1
TOL = dict(delta=4 * 4.461e-08, gamma=4 * 2.146e-07, vega=4 * 7.691e-08, rho=4 * 4.222e-08, theta=4 * 1.413e-07,
           epsilon=4 * 3.752e-08)
CAP = 0.01  # of the Greek's standard error
SUM = 1e-9  # the project's standing contract for a reordered float64 sum
H = 0.01


def divs_at(steps, T, N):
    return dc.dividends_at(steps, T, N)


def compare(ctx, p, q, divs, h, betas=None, label=""):
    """one call against the restatement on the device's own inputs -> (out, ref, mats, results of the three pricings)"""
    mats, res, Z = gc.device_inputs(ctx, p, q, divs, h)
    out = ctx.price_american_dividend_greeks(p, q, divs, bump=h, betas=betas, want_betas=True)
    ref = gc.restate(p, q, divs, h, mats, Z, out["betas"])
    assert ref["ties"] == [0, 0, 0], "a decision within 1e-10 K of its continuation value: not a case for exact counts"
    for k in ("n_exercised", "n_zero", "n_exercised_up", "n_exercised_down"):
        assert out[k] == ref[k], (label, k, out[k], ref[k])
    for k in ("price", "price_up", "price_down"):
        assert abs(out[k] - ref[k]) <= SUM * abs(ref[k]), (label, k, out[k], ref[k])
    gbm = Z is not None
    err = gc.rel_errors(out, ref, gbm)
    print("MEASURED", label, " ".join(f"{g}={e:.3e}" for g, e in err.items()),
          " ".join(f"se/|{g}|={ref['se_' + g] / abs(ref[g]):.3e}" for g in err if ref[g] != 0.0))
    for g, e in err.items():
        assert e <= TOL[g], (label, g, out[g], ref[g], e)
        assert TOL[g] * abs(ref[g]) <= CAP * ref["se_" + g], (label, g, "the tolerance is not below 1 % of the standard error")
        assert abs(out["se_" + g] - ref["se_" + g]) <= 1e-3 * ref["se_" + g] + 1e-300, (label, "se_" + g)
    if not gbm:
        assert all(math.isnan(out[k]) for k in ("vega", "rho", "theta", "epsilon", "se_vega", "se_rho", "se_theta", "se_epsilon"))
    assert out["folded"] == 0 and out["ms_pass2"] == 0.0 and out["ms_greeks"] > 0.0 and out["bump"] == h
    return out, ref, mats, res


CASES = []
for i, (model, sched) in enumerate((m, s) for m in gc.MODELS for s in gc.SCHEDULES):
    CASES.append(dict(model=model, sched=sched, N=(5, 7, 12)[i % 3], M=(gc.RAGGED, 4096)[i % 2], is_put=i % 4 < 2,
                      q=0.02 if i % 3 == 0 else 0.0, seed=100 + i))


def _id(c):
    return f"{c['model']}-{c['sched']}-N{c['N']}-M{c['M']}-{'put' if c['is_put'] else 'call'}"


def _params(c, **kw):
    return gc.make_params(c["model"], is_put=c["is_put"], N=c["N"], M=c["M"], seed=c["seed"], sigma=0.25, **kw)


# ------------------------------------------------------------------ 1. the scenario paths are the generator's
@pytest.mark.parametrize("c", CASES[2::5], ids=[_id(c) for c in CASES[2::5]])
def test_scenario_paths_are_the_generators(ctx, c):
    N = c["N"]
    divs = divs_at(gc.SCHEDULES[c["sched"]](N), 1.0, N)
    p = _params(c)
    for step in (0, 1, N - 1, (N + 1) // 2):  # 0: nowhere, every chain ends at N
        out, ref, mats, _ = compare(ctx, p, c["q"], divs, H, betas=gc.stop_at(N, step), label=f"stop{step}-{_id(c)}")
        assert out["sum_nitm"] == 0
        if 1 <= step < N:
            S = mats[0][step].astype(np.float64)
            assert out["n_exercised"] == int(((p.K - S if p.is_put else S - p.K) > 0.0).sum())
        else:
            assert out["n_exercised"] == 0


# ------------------------------------------------------------------ 2. + 3. the base pricing and the Greeks, fitted policy
@pytest.mark.parametrize("c", CASES, ids=[_id(c) for c in CASES])
def test_pricing_and_greeks_against_the_restatement(ctx, c):
    N = c["N"]
    divs = divs_at(gc.SCHEDULES[c["sched"]](N), 1.0, N)
    p = _params(c)
    out, ref, mats, res = compare(ctx, p, c["q"], divs, H, label=_id(c))
    base = res[0]
    assert (out["n_exercised"], out["n_zero"], out["sum_nitm"]) == (base["n_exercised"], base["n_zero"], base["sum_nitm"])
    assert abs(out["price"] - base["price"]) <= SUM * abs(base["price"]), (out["price"], base["price"], ref["price"])
    Sd = ctx.to_device(mats[0])
    try:
        fit = ctx.lsm_poly(Sd, p.K, p.r, p.T, bool(p.is_put), "two_pass")
    finally:
        Sd.free()
    np.testing.assert_array_equal(out["betas"][:, :3].view(np.uint64), np.ascontiguousarray(fit["betas"]).view(np.uint64))
    np.testing.assert_array_equal(out["betas"][:, 3].astype(np.int64), fit["nitm"])
    steps = sorted({k for k, _, _ in gc.SCHEDULES[c["sched"]](N)})
    assert (out["n_div_steps"], out["first_div_step"]) == (len(steps), steps[0])
    if c["sched"] == "floor":  # 7: floored and live paths together
        dead = mats[0][N] == 0.0
        assert dead.any() and not dead.all()


# ------------------------------------------------------------------ 4. no dividends: omc_price_american_greeks
@pytest.mark.parametrize("model,is_put,N,M", [("gbm", True, 7, gc.RAGGED), ("gbm", False, 12, 4096), ("heston0", True, 5, 4096),
                                              ("heston3", False, 7, gc.RAGGED)])
def test_without_dividends_it_is_the_vanilla_greeks_sweep(ctx, model, is_put, N, M):
    p = gc.make_params(model, is_put=is_put, N=N, M=M, seed=77, sigma=0.25)
    out = ctx.price_american_dividend_greeks(p, 0.0, [], bump=H, want_betas=True)
    ctx.set_option("fold_antithetic", 0)
    try:
        van = ctx.price_american_greeks(p, bump=H, want_betas=True)
    finally:
        ctx.set_option("fold_antithetic", 1)
    assert van["folded"] == 0 and (out["n_div_steps"], out["first_div_step"]) == (0, 0)
    np.testing.assert_array_equal(out["betas"].view(np.uint64), van["betas"].view(np.uint64))
    for k in ("n_exercised", "n_zero", "sum_nitm", "n_exercised_up", "n_exercised_down"):
        assert out[k] == van[k], k
    assert abs(out["price"] - van["price"]) <= SUM * abs(van["price"])  # the same spots, another sum order
    # the vanilla sweep's bumped spot is lambda s in float64, this sweep's a float32 path started at (float)(lambda S0): they
    # differ by float32 rounding, 6e-8 of a spot near 100 -- 6e-6 -- times |delta| < 1 on a price above 3: below 2e-6
    for k in ("price_up", "price_down"):
        assert van[k] > 3.0 and abs(out[k] - van[k]) <= 2e-6 * abs(van[k]), k
    gbm = model == "gbm"
    names = ("delta", "gamma", "vega", "rho", "theta") if gbm else ("delta", "gamma")
    err = gc.rel_errors({g: out[g] for g in names}, {g: van[g] for g in names}, gbm, names)
    print("MEASURED", f"vanilla-{model}-N{N}", " ".join(f"{g}={e:.3e}" for g, e in err.items()))
    for g, e in err.items():
        assert e <= TOL[g], (g, out[g], van[g], e)
        assert TOL[g] * abs(van[g]) <= CAP * van["se_" + g], g
    if gbm:  # without discrete dividends dS/dq = -dS/dr = -k dt S: epsilon is the spot part of rho with the sign turned
        assert math.isfinite(out["epsilon"]) and out["epsilon"] * out["delta"] <= 0.0


# ------------------------------------------------------------------ 5. a cash dividend of amount 0
@pytest.mark.parametrize("model", ["gbm", "heston1"])
def test_a_cash_dividend_of_zero_changes_no_bit(ctx, model):
    p = gc.make_params(model, N=7, M=gc.RAGGED, seed=9, sigma=0.25)
    divs = divs_at([(2, 1.0, gc.C)], 1.0, 7)
    a = ctx.price_american_dividend_greeks(p, 0.01, divs, bump=H, want_betas=True)
    b = ctx.price_american_dividend_greeks(p, 0.01, divs + divs_at([(4, 0.0, gc.C)], 1.0, 7), bump=H, want_betas=True)
    assert (a["n_div_steps"], b["n_div_steps"]) == (1, 2)
    for d in (a, b):
        d.pop("n_div_steps"), d.pop("first_div_step")
    assert cat.diff(cat.flat(a), cat.flat(b)) == []


# ------------------------------------------------------------------ 6. the European policy: Black-Scholes-Merton
def _bsm_quirk(S0, K, r, q, sig, T, N, deltas, is_put):
    """the closed form at spot S0 prod(1 - delta) and yield q, valued at t = dt as the two-pass flow values (D[k-1])"""
    return math.exp(r * T / N) * dr.bsm(S0 * float(np.prod([1.0 - d for d in deltas])), K, r, q, sig, T, is_put)


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
def test_european_policy_is_black_scholes_merton(ctx, is_put):
    S0, K, r, q, sig, T, N, M = 100.0, 100.0, 0.05, 0.03, 0.2, 1.0, 12, 16384
    deltas = [0.02, 0.03, 0.01]
    steps = [(3, deltas[0], gc.P), (7, deltas[1], gc.P), (12, deltas[2], gc.P)]
    p = gc.make_params("gbm", is_put=is_put, S0=S0, K=K, r=r, sigma=sig, T=T, N=N, M=M, seed=42)
    out, ref, _, _ = compare(ctx, p, q, divs_at(steps, T, N), H, betas=gc.stop_at(N, 0), label=f"european-{is_put}")
    x0 = dict(S0=S0, r=r, q=q, sig=sig)

    def f(**kw):
        a = dict(x0, **kw)
        return _bsm_quirk(a["S0"], K, a["r"], a["q"], a["sig"], T, N, deltas, is_put)

    def d(name):  # the closed form is analytic: a central difference of 1e-6 relative is good to 1e-9
        e = 1e-6 * x0[name]
        return (f(**{name: x0[name] + e}) - f(**{name: x0[name] - e})) / (2.0 * e)

    want = dict(price=f(), delta=d("S0"), vega=d("sig"), rho=d("r"), epsilon=d("q"))
    se = dict(ref, se_price=math.sqrt(max(ref["sumsq"] / M - ref["price"] ** 2, 0.0) / M))
    for k, w in want.items():
        print("EUROPEAN", k, out[k], ref[k], w, se["se_" + k])
        assert abs(ref[k] - w) <= 3.0 * se["se_" + k], (k, ref[k], w, se["se_" + k])
        assert abs(out[k] - w) <= 4.0 * se["se_" + k], (k, out[k], w, se["se_" + k])


# ------------------------------------------------------------------ 7. a schedule that floors every path
@pytest.mark.parametrize("model,is_put", [("gbm", True), ("gbm", False), ("heston0", True)])
def test_a_schedule_that_floors_every_path_has_no_delta(ctx, model, is_put):
    N = 7
    p = gc.make_params(model, is_put=is_put, N=N, M=gc.RAGGED, seed=5, sigma=0.25)
    for betas in (gc.stop_at(N, 0), gc.stop_at(N, 4)):
        out = ctx.price_american_dividend_greeks(p, 0.0, divs_at(gc.FLOOR_ALL, 1.0, N), bump=H, betas=betas)
        assert out["delta"] == 0.0 and out["gamma"] == 0.0 and out["se_delta"] == 0.0
        if model == "gbm":
            assert out["vega"] == 0.0 and out["epsilon"] == 0.0
        want = p.K * math.exp(-p.r * p.T / N * ((4 if betas[4, 3] else N) - 1)) if is_put else 0.0  # the payoff K at spot 0
        assert abs(out["price"] - want) <= SUM * max(want, 1.0)


# ------------------------------------------------------------------ 8. identical bits
@pytest.mark.parametrize("model", ["gbm", "heston3"])
def test_identical_calls_return_identical_bits(ctx, model):
    p = gc.make_params(model, N=12, M=4096, seed=31, sigma=0.25)
    divs = divs_at(gc.SCHEDULES["mixed"](12), 1.0, 12)
    a = ctx.price_american_dividend_greeks(p, 0.02, divs, bump=H, want_betas=True)
    b = ctx.price_american_dividend_greeks(p, 0.02, divs, bump=H, want_betas=True)
    assert cat.diff(cat.flat(a), cat.flat(b)) == []
    g = ctx.price_american_dividend_greeks(p, 0.02, divs, bump=H, betas=a["betas"], want_betas=True)
    assert g["sum_nitm"] == 0 and a["sum_nitm"] > 0
    fa, fg = cat.flat(a), cat.flat(g)
    for d in (fa, fg):
        d.pop("sum_nitm")
    assert cat.diff(fa, fg) == []


# ------------------------------------------------------------------ 9. the C error codes
def test_error_codes(ctx):
    lib = ctx.lib
    p = gc.make_params("gbm", N=7, M=2048, seed=1)
    out = _ffi.DivGreeks()

    def call(pp=p, q=0.0, divs=((0.5, 1.0),), n=None, bump=0.01, res=out, handle=None):
        arr, cnt = _ffi.dividend_array(divs)
        return lib.omc_price_american_div_greeks(handle or ctx.handle, C.byref(pp), float(q), arr, cnt if n is None else n,
                                                 float(bump), None, None, C.byref(res) if res is not None else None)

    assert call() == 0
    assert [call(bump=b) for b in (0.0, 0.6, math.nan, -0.01)] == [-4] * 4
    assert call(bump=0.5) == 0
    assert call(res=None) == -7
    assert call(q=math.nan) == -17 and call(n=-1) == -18 and call(divs=(), n=2) == -19
    assert call(divs=((0.0, 1.0),)) == -20 and call(divs=((1.5, 1.0),)) == -20
    assert call(divs=((0.5, -1.0),)) == -21 and call(divs=((0.5, math.inf),)) == -21
    assert call(divs=((0.5, 1.0, "proportional"),)) == -22 and call(divs=((0.5, 0.1, 5),)) == -23
    assert call(pp=dc.with_(p, antithetic=0)) == -24
    assert call(pp=dc.with_(p, semantics=_ffi.SEMANTICS["reference"])) == -11
    assert call(pp=dc.with_(p, n_paths=2047)) == -3
    # the schedule's refusals come before the bump's
    assert call(q=math.nan, bump=0.0) == -17
    c = _ffi.Context(0)
    try:
        c.set_allreduce_hook(lambda dptr, count: None)
        assert call(handle=c.handle) == -10
        with pytest.raises(ValueError):
            c.price_american_dividend_greeks(p, 0.0, [(0.5, 1.0)])
        c.set_allreduce_hook(None)
        assert call(handle=c.handle) == 0
    finally:
        c.close()
    with pytest.raises(ValueError):
        ctx.price_american_dividend_greeks(p, 0.0, [], betas=np.zeros((5, 4)))
    assert call() == 0  # and the context still prices


def test_facade_returns_the_ffi_numbers(ctx):
    from options_model_amd import DividendGreeksResult, price_american_dividend_greeks
    divs = [(0.2, 0.5), (0.7, 0.01, "proportional"), (0.45, 0.75, "cash")]
    for model in ("GBM", "Heston"):
        r = price_american_dividend_greeks(100.0, 100.0, 0.05, 0.2, 1.0, 4096, 12, dividend_yield=0.01, dividends=divs,
                                           model=model, option_type="put", seed=5, bump=0.02, ctx=ctx)
        p = _ffi.make_params(model=model.lower(), is_put=True, semantics="two_pass", n_paths=4096, n_steps=12, S0=100.0, K=100.0,
                             r=0.05, sigma=0.2, T=1.0, seed=5, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
        o = ctx.price_american_dividend_greeks(p, 0.01, divs, bump=0.02, want_betas=True)
        assert isinstance(r, DividendGreeksResult) and float(r) == r.price == o["price"]
        for k in ("delta", "gamma", "se_delta", "se_gamma", "price_up", "price_down", "n_exercised_up", "n_exercised_down", "bump"):
            assert getattr(r, k) == o[k], k
        for k in ("vega", "rho", "theta", "epsilon", "se_epsilon"):
            assert getattr(r, k) == o[k] or (math.isnan(getattr(r, k)) and math.isnan(o[k])), k
        assert (r.dividend_steps, r.first_dividend_step, r.folded, r.n_paths) == (3, 3, False, 4096)
        np.testing.assert_array_equal(r.betas, o["betas"])

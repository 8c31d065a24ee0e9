"""The six bounds facades of options_model_amd.api against the Context call they stand on: one call each at the smallest
sizes, then the direct Context.price_*bounds* call on the same context with the omc_params the facade is documented to build
(restated here with _ffi.make_params).  Every common field of the result equals the dict's value exactly, `betas` bit for
bit, and every law field is what the arguments say.  The Context calls themselves are held against their restatements by
the suites of the laws; this ties the facades' one result builder to them."""
import dataclasses

import numpy as np
import pytest

from options_model_amd import _ffi, api

pytestmark = pytest.mark.gpu

N, M = 4, 4096
SIZES = dict(policy="textbook", n_lower=2048, n_outer=64, n_inner=16)
K, R, SIG, T, SEED, STREAM = 100.0, 0.05, 0.2, 1.0, 7, 5
HP = dict(v0=0.05, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
COMMON = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
          "inner_path_steps")
SHARED = [f.name for f in dataclasses.fields(api.BoundsResult)]


def _params(model, is_put=True, S0=100.0, sigma=SIG):
    """what a facade hands to its Context call: two-pass flow, antithetic pairs; under Heston the scheme and the five"""
    common = dict(is_put=is_put, semantics="two_pass", antithetic=True, n_paths=M, n_steps=N, S0=S0, K=K, r=R, T=T, seed=SEED,
                  stream=STREAM)
    if model == "heston":
        return _ffi.make_params(model="heston", heston_scheme="full_truncation", sigma=sigma or 0.0, **HP, **common)
    return _ffi.make_params(sigma=sigma, **common)


def _dates(every):
    return len([t for t in range(1, N + 1) if every < 2 or (N - t) % every == 0])


def _same(res, cls, out, option_type, cols, **law):
    """res is a `cls` with the dict's values, the policy and the option type it was asked for, and the law's own fields"""
    assert type(res) is cls
    for k in COMMON:
        assert getattr(res, k) == out[k] and type(getattr(res, k)) is type(out[k]), k
    assert res.lower > 0.0 and res.upper >= res.lower - 4 * (res.se_lower + res.se_upper) and res.inner_path_steps > 0
    assert res.betas.shape == out["betas"].shape == (N + 1, cols) and res.betas.dtype == out["betas"].dtype == np.float64
    assert np.array_equal(res.betas.view(np.uint64), out["betas"].view(np.uint64)) and res.betas.any()
    assert res.policy == "textbook" and res.option_type == option_type
    assert sorted(res.timings_ms) == ["fit", "lower", "total", "upper"]
    want = dict(exercise_every=0, n_exercise_dates=0, control_variate=False, suboptimality_check="off")
    want.update(law)
    got = {f.name: getattr(res, f.name) for f in dataclasses.fields(res)}
    assert sorted(got) == sorted(set(SHARED) | set(want))  # no field of the result is left unchecked
    for k, v in want.items():
        assert got[k] == v and type(got[k]) is type(v), (k, got[k], v)


def test_gbm(ctx):
    options = (ctx._bounds_every, ctx._bounds_cv, ctx._bounds_check)
    res =api.price_american_bounds(100.0, K, R, SIG, T, M + 1, N, option_type="call", seed=SEED, stream=STREAM, ctx=ctx,
                                    control_variate=True, exercise_every=2, **SIZES)
    out = ctx.price_american_bounds(_params("gbm", is_put=False), exercise_every=2, control_variate=True, **SIZES)
    _same(res, api.BoundsResult, out, "call", 4, exercise_every=2, n_exercise_dates=_dates(2), control_variate=True)
    assert _dates(2) == 2 and (ctx._bounds_every, ctx._bounds_cv, ctx._bounds_check) == options  # (set for the call only)


def test_heston(ctx):
    res = api.price_american_bounds_heston(100.0, K, R, T, M, N, heston_params=HP, heston_scheme="full_truncation", seed=SEED,
                                           stream=STREAM, ctx=ctx, regressors="spot+variance", **SIZES)
    out = ctx.price_american_bounds_heston(_params("heston", sigma=None), regressors="spot+variance", **SIZES)
    _same(res, api.HestonBoundsResult, out, "put", 8, regressors="spot+variance", variance_scale=0.05,
          n_exercise_dates=_dates(0))
    assert _dates(0) == N


@pytest.mark.parametrize("model", ["gbm", "heston"])
def test_jumps(ctx, model):
    res = api.price_american_bounds_jumps(100.0, K, R, SIG, T, M, N, 1.5, jump_mean=-0.1, jump_vol=0.15, dividend_yield=0.01,
                                          model=model.upper(), heston_params=HP, heston_scheme="full_truncation", seed=SEED,
                                          stream=STREAM, ctx=ctx, suboptimality_check="payoff", **SIZES)
    out = ctx.price_american_bounds_jump(_params(model), (1.5, -0.1, 0.15), 0.01, suboptimality_check="payoff", **SIZES)
    _same(res, api.JumpBoundsResult, out, "put", 4, n_exercise_dates=N, suboptimality_check="payoff", jump_intensity=1.5,
          jump_mean=-0.1, jump_vol=0.15, dividend_yield=0.01, model=model)


@pytest.mark.parametrize("model", ["gbm", "heston"])
def test_dividends(ctx, model):
    divs = [(0.4, 1.0), (0.8, 0.02, "proportional")]  # two ex-dividend steps of the grid of 4, the first of them step 2
    res = api.price_american_bounds_dividends(100.0, K, R, SIG, T, M, N, dividend_yield=0.01, dividends=divs,
                                              model=model.upper(), heston_params=HP, heston_scheme="full_truncation", seed=SEED,
                                              stream=STREAM, ctx=ctx, exercise_every=3, **SIZES)
    p = _params(model)
    out = ctx.price_american_bounds_div(p, 0.01, divs, exercise_every=3, **SIZES)
    priced = ctx.price_american_div(p, 0.01, divs)  # the library's own count of the ex-dividend steps
    assert (priced["n_div_steps"], priced["first_div_step"]) == (2, 2)
    _same(res, api.DividendBoundsResult, out, "put", 4, exercise_every=3, n_exercise_dates=_dates(3), dividend_yield=0.01,
          n_div_steps=priced["n_div_steps"], first_div_step=priced["first_div_step"], model=model)
    assert _dates(3) == 2


@pytest.mark.parametrize("model", ["gbm", "heston"])
def test_barrier(ctx, model):
    res = api.price_barrier_bounds(100.0, K, R, SIG, T, M, N, 85, barrier_type="down-and-out", model=model.upper(),
                                   heston_params=HP, heston_scheme="full_truncation", exercise_every=2, seed=SEED, stream=STREAM,
                                   ctx=ctx, **SIZES)
    out = ctx.price_barrier_bounds(_params(model), "down-and-out", 85.0, exercise_every=2, **SIZES)
    _same(res, api.BarrierBoundsResult, out, "put", 4, exercise_every=2, n_exercise_dates=2, barrier=85.0,
          barrier_type="down-and-out", monitoring="discrete", model=model)


def test_basket(ctx):
    spots, sigmas, rho = [100.0, 95.0], [0.2, 0.3], [[1.0, 0.3], [0.3, 1.0]]
    res = api.price_american_basket_bounds(spots, K, R, sigmas, T, M, N, correlation=rho, kind="best-of", option_type="call",
                                           seed=SEED, stream=STREAM, ctx=ctx, regressors="index+runner-up", **SIZES)
    b = _ffi.make_basket(spots, sigmas, [0.0, 0.0], [1.0, 1.0], rho, "best-of")
    out = ctx.price_american_basket_bounds(_params("gbm", is_put=False, sigma=sigmas[0]), b, regressors="index+runner-up",
                                           **SIZES)
    assert (out["index0"], out["n_assets"], out["kind"]) == (100.0, 2, _ffi.BASKET_KINDS["best-of"])
    _same(res, api.BasketBoundsResult, out, "call", 8, index0=100.0, n_assets=2, kind="best-of",
          regressors="index+runner-up")

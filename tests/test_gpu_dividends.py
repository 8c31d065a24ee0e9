"""Dividend yield and discrete dividends (omc_price_american_div, options_model_amd/csrc/omc_dividend.hip; DESIGN.md
section 14).

What is compared, and how tightly:
  * q = 0, no dividends                      `base` is omc_price_american's result, bit for bit
  * yield only, folded storage               the folded oracle at drift r - q, discount r: counts identical, price 1e-9
  * a zero-amount dividend                   the matrix is the vanilla generator's at drift r - q, bit for bit; with a
                                             real schedule the rows before the first dividend step are
  * the matrix with dividends                tests/helpers/dividend_ref.apply on the vanilla DEVICE matrix: rel 2e-5 GBM,
                                             5e-5 Heston, atol = rtol * the column's largest vanilla spot (n_steps <= 64)
  * the price                                the C oracle's two-pass flow on the device's own matrix: counts identical,
                                             price rel 1e-9 -- also with a cash dividend that takes a fifth of the paths to 0
  * known answers                            the European value of the device matrix within 4 standard errors of
                                             Black-Scholes-Merton (yield, proportional dividends, both)
"""
import math

import numpy as np
import pytest

from helpers import dividend_ref as dr
from helpers.call_catalogue import diff, flat
from oracle import cpu as orc
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

S0, K, R, SIG, T = 100.0, 100.0, 0.05, 0.2, 1.0
HES = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
MODELS = [("gbm", 0), ("heston", 0), ("heston", 1), ("heston", 2)]
# the smallest shapes that reach every code path of the generator
SHAPES = [(20_008, 31),   # VEC 4, last workgroup partly filled
          (20_004, 37),   # 10,002 pairs: VEC 2
          (20_002, 50),   # 10,001 pairs: VEC 1
          (1_026, 7),     # steps not a multiple of a Philox block
          (2, 3),         # one pair
          (4_096, 1)]     # one step, the dividend on it
RTOL = {"gbm": 2e-5, "heston": 5e-5}
KEYS = ("price", "sum", "sumsq", "std", "zero_prob", "n_paths", "n_exercised", "n_zero", "sum_nitm", "folded")


def params(model="gbm", scheme=0, is_put=True, M=4096, N=50, seed=42, stream=3, pair_offset=0, **kw):
    kw = {**dict(S0=S0, K=K, r=R, sigma=SIG, T=T), **HES, **kw}
    return _ffi.make_params(model=model, heston_scheme=scheme, is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N,
                            seed=seed, stream=stream, pair_offset=pair_offset, **kw)


def vanilla(ctx, p, q):
    """the vanilla generator's matrix at drift r - q"""
    if p.model == 1:
        S = ctx.heston_paths(p.n_paths, p.n_steps, p.S0, p.r - q, p.T, p.v0, p.kappa, p.theta, p.xi, p.rho, p.seed, p.stream,
                             p.pair_offset, scheme=p.heston_scheme)
    else:
        S = ctx.gbm_paths(p.n_paths, p.n_steps, p.S0, p.r - q, p.sigma, p.T, p.seed, p.stream, p.pair_offset)
    out = S.to_host()
    S.free()
    return out


def priced(ctx, p, q, divs):
    """-> (result dict, the path matrix the call wrote)"""
    keep = ctx.empty((p.n_steps + 1, p.n_paths), np.float32)
    out = ctx.price_american_div(p, q, divs, S_keep=keep)
    S = keep.to_host()
    keep.free()
    return out, S


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def at_steps(p, steps, amounts):
    """dividends that go ex on the given steps: times in the middle of the interval each step ends"""
    dt = p.T / p.n_steps
    return [((k - 0.5) * dt,) + tuple(a) for k, a in zip(steps, amounts)]


def mixed_schedule(p, model):
    """cash and proportional dividends on steps 1, N and both sides of a Philox block boundary (GBM: 4 normals = 4 steps
    per block, Heston: 2 steps), two of them on one step"""
    N = p.n_steps
    edge = (4, 5) if model == "gbm" else (2, 3)
    steps = sorted({k for k in (1,) + edge + (N,) if 1 <= k <= N})
    amounts = [(0.9, "cash"), (0.015, "proportional"), (1.3, "cash"), (0.02, "proportional")][:len(steps)]
    divs = at_steps(p, steps, amounts)
    divs.append((divs[-1][0], 0.4, "cash"))  # a second dividend on the last of these steps
    return divs[::-1], steps  # (unsorted on purpose)


def check_matrix(ctx, p, q, divs, S, model):
    """check 4: the matrix against the restatement on the vanilla device matrix; rows before the first dividend step
    carry the vanilla bits"""
    V = vanilla(ctx, p, q)
    mul, cash, has = dr.schedule(p.T, p.n_steps, divs)
    ref = dr.apply(V, mul, cash, has)
    ok, worst = dr.close(S, ref, V, RTOL[model])
    assert ok, (model, p.n_paths, p.n_steps, worst)
    first = int(np.argmax(has)) if has.any() else p.n_steps + 1
    assert np.array_equal(bits(S[:first]), bits(V[:first]))
    return V, has


def check_price(out, S, p):
    """check 5: the C oracle's two-pass flow on the device's own matrix"""
    ref = orc.lsm_poly(S, p.K, p.r, p.T, bool(p.is_put), "two_pass")
    same = (abs(out["price"] - ref["price"]) <= 1e-9 * max(abs(ref["price"]), 1e-12) + 1e-15
            and (out["n_exercised"], out["n_zero"], out["sum_nitm"]) == (ref["n_exercised"], ref["n_zero"], ref["sum_nitm"]))
    if not same:
        # an exact tie (a decision within 1e-10 K of the continuation value) is the one thing two correct implementations
        # may decide differently, as in tests/test_gpu_fuzz.py; anything else is a failure
        from test_gpu_fuzz import _smallest_margin
        margin = _smallest_margin(S, p.K, p.r, p.T, bool(p.is_put), "two_pass")
        assert margin <= 1e-10, (margin, {k: out[k] for k in KEYS}, {k: ref[k] for k in ("price", "n_exercised", "n_zero", "sum_nitm")})
    return ref


# ------------------------------------------------------------------ 1. nothing paid: omc_price_american
@pytest.mark.parametrize("M,N,folded", [(20_004, 37, 0), (131_072, 12, 1)])
def test_no_yield_no_dividends_is_price_american_bit_for_bit(ctx, M, N, folded):
    for model, scheme in (("gbm", 0), ("heston", 1)):
        for is_put in (True, False):
            p = params(model, scheme, is_put=is_put, M=M, N=N)
            a = ctx.price_american(p)
            b = ctx.price_american_div(p, 0.0, [])
            assert [a[k] for k in KEYS] == [b[k] for k in KEYS], (model, is_put)
            assert b["folded"] == (folded if model == "gbm" else 0)
            assert (b["n_div_steps"], b["first_div_step"]) == (0, 0)


# ------------------------------------------------------------------ 2. yield only on folded storage
@pytest.fixture
def fctx(ctx):
    ctx.set_option("fold_antithetic", 2)
    yield ctx
    ctx.set_option("fold_antithetic", 1)


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("M,N", SHAPES[1:4] + [(131_072, 12)])
def test_yield_only_equals_the_folded_oracle(fctx, M, N, is_put):
    """(q = 0.02, not the 0.03 of the known-answer tests: with r = 0.05 and sigma = 0.2 a yield of 0.03 makes the log-drift
    r - q - sigma^2 / 2 zero, so S S' = S0^2 = K^2 and a stored spot that equals K exactly leaves its partner's payoff
    an exact tie at 0, which the folded sweep and the oracle round differently -- 1 of 720,896 in-the-money rows at
    131,072 x 12; the same holds for omc_price_american at r = 0.02, it is no property of the yield)"""
    q = 0.02
    p = params(is_put=is_put, M=M, N=N, seed=2024, stream=5)
    r = fctx.price_american_div(p, q, [])
    half = fctx.gbm_paths(M // 2, N, p.S0, p.r - q, p.sigma, p.T, p.seed, p.stream, p.pair_offset, antithetic=False)
    c0, g = orc.fold_constants(p.S0, p.K, p.r - q, p.sigma, p.T, N)
    o = orc.lsm_two_pass_folded(half.to_host(), p.K, p.r, p.T, is_put, c0, g)
    half.free()
    assert r["folded"] == 1 and r["n_paths"] == M and r["n_div_steps"] == 0
    assert (r["sum_nitm"], r["n_exercised"], r["n_zero"]) == (o["sum_nitm"], o["n_exercised"], o["n_zero"])
    assert r["price"] == pytest.approx(o["price"], rel=1e-9, abs=1e-300)
    assert r["sumsq"] == pytest.approx(o["sumsq"], rel=1e-9, abs=1e-300)


def test_yield_makes_the_call_worth_exercising(ctx):
    """without dividends an American call is never exercised early by an exact rule; a yield above r makes it so"""
    p = params(is_put=False, M=65_536, N=20)
    lo, hi = ctx.price_american_div(p, 0.0, []), ctx.price_american_div(p, 0.08, [])
    assert hi["price"] < lo["price"] and hi["n_exercised"] > lo["n_exercised"]


# ------------------------------------------------------------------ 3. the vanilla bits
@pytest.mark.parametrize("model,scheme", MODELS)
@pytest.mark.parametrize("M,N", SHAPES[:4])
def test_a_zero_dividend_changes_no_bit(ctx, model, scheme, M, N):
    q = 0.02
    p = params(model, scheme, M=M, N=N, seed=9, stream=1, pair_offset=12345)
    V = vanilla(ctx, p, q)
    for kind in ("cash", "proportional"):
        out, S = priced(ctx, p, q, at_steps(p, [3], [(0.0, kind)]))
        assert np.array_equal(bits(S), bits(V)), (model, scheme, kind)
        assert (out["folded"], out["n_div_steps"], out["first_div_step"]) == (0, 1, 3)
    out, S = priced(ctx, p, q, at_steps(p, [5, 6], [(1.0, "cash"), (0.01, "proportional")]))
    assert np.array_equal(bits(S[:5]), bits(V[:5])) and not np.array_equal(bits(S[5]), bits(V[5]))
    assert (out["n_div_steps"], out["first_div_step"]) == (2, 5)


# ------------------------------------------------------------------ 4. + 5. restatement and price, every shape and model
@pytest.mark.parametrize("model,scheme", MODELS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_matrix_matches_the_restatement_and_price_the_oracle(ctx, model, scheme, M, N):
    q = 0.025 if scheme != 1 else -0.01
    for is_put in (True, False):
        p = params(model, scheme, is_put=is_put, M=M, N=N, seed=77, stream=2)
        divs, steps = mixed_schedule(p, model)
        out, S = priced(ctx, p, q, divs)
        _, has = check_matrix(ctx, p, q, divs, S, model)
        assert list(np.nonzero(has)[0]) == steps and out["n_div_steps"] == len(steps) and out["first_div_step"] == steps[0]
        assert out["folded"] == 0 and out["n_paths"] == M
        check_price(out, S, p)


def test_a_cash_dividend_that_takes_paths_to_zero(ctx):
    """cash = 0.8 S0 at mid-life, sigma = 0.4: about a fifth of the paths cannot cover it and sit at exactly 0 from that
    step on (CPU, 200,000 C-oracle paths at these parameters: 24.8 % GBM, 23.9 % Heston) -- zeros are ordinary spots for the sweeps
    (DESIGN.md 14.3), and the regression keeps paths on both sides"""
    q, N, M = 0.03, 20, 40_000
    for model, scheme in (("gbm", 0), ("heston", 0)):
        for is_put in (True, False):
            p = params(model, scheme, is_put=is_put, M=M, N=N, sigma=0.4, v0=0.16, theta=0.16, seed=31, stream=4)
            divs = at_steps(p, [N // 2], [(0.8 * S0, "cash")])
            out, S = priced(ctx, p, q, divs)
            zero = S[N // 2] == 0.0
            share = zero.mean()
            print(f"{model} put={is_put}: {100 * share:.2f} % of the columns at 0 from step {N // 2}")
            assert 0.01 <= share <= 0.50
            assert np.all(S[N // 2:, zero] == 0.0) and np.all(S[:N // 2] > 0.0)
            check_matrix(ctx, p, q, divs, S, model)
            ref = check_price(out, S, p)
            assert math.isfinite(out["price"]) and out["price"] > 0.0 and ref["n_exercised"] > 0


# ------------------------------------------------------------------ 6. determinism, S_keep
@pytest.mark.parametrize("model,scheme", [("gbm", 0), ("heston", 2)])
def test_keeping_the_matrix_changes_nothing_and_calls_repeat(ctx, model, scheme):
    p = params(model, scheme, M=20_004, N=37)
    divs, _ = mixed_schedule(p, model)
    a = ctx.price_american_div(p, 0.02, divs)
    b, S = priced(ctx, p, 0.02, divs)
    c = ctx.price_american_div(p, 0.02, divs)
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS] == [c[k] for k in KEYS]
    # a matrix with a leading dimension of its own (odd: scalar-width stores in the generator, and scalar-width loads in
    # the sweeps, whose float64 sums then run in another order): the same spots and decisions, the price to 1e-12
    keep = ctx.empty((p.n_steps + 1, p.n_paths + 3), np.float32)
    d = ctx.price_american_div(p, 0.02, divs, S_keep=keep)
    assert [a[k] for k in KEYS[5:]] == [d[k] for k in KEYS[5:]] and d["price"] == pytest.approx(a["price"], rel=1e-12)
    assert np.array_equal(bits(keep.to_host()[:, :p.n_paths]), bits(S))
    keep.free()
    # yield only with S_keep: full storage, the vanilla matrix at r - q
    e, Sy = priced(ctx, p, 0.02, [])
    assert e["folded"] == 0 and np.array_equal(bits(Sy), bits(vanilla(ctx, p, 0.02)))


# ------------------------------------------------------------------ 7. known answers
@pytest.mark.parametrize("q,props", [(0.03, ()), (0.0, (0.02, 0.035)), (0.03, (0.02, 0.035))], ids=["yield", "proportional", "both"])
def test_european_value_of_the_matrix_is_black_scholes_merton(ctx, q, props):
    M, N = 400_000, 16
    p = params(M=M, N=N, seed=123, stream=8)
    divs = [(0.3 + 0.5 * i, d, "proportional") for i, d in enumerate(props)]
    _, S = priced(ctx, p, q, divs)
    spot = S0 * math.prod(1.0 - d for d in props)
    for is_put in (True, False):
        s, s2 = orc.european_from_paths(S, K, R, T, is_put)
        mean = s / M
        se = math.sqrt(max(s2 / M - mean * mean, 0.0) / M)
        ref = dr.bsm(spot, K, R, q, SIG, T, is_put)
        print(f"q={q} props={props} put={is_put}: device {mean:.5f} +- {se:.5f}  bsm {ref:.5f}")
        assert abs(mean - ref) <= 4.0 * se


# ------------------------------------------------------------------ 8. facade, refusals
def test_facade_returns_the_ffi_numbers(ctx):
    from options_model_amd import DividendResult, price_american_dividends
    divs = [(0.2, 0.5), (0.7, 0.01, "proportional"), (0.45, 0.75, "cash")]
    for model in ("GBM", "Heston"):
        for opt in ("put", "call"):
            r = price_american_dividends(S0, K, R, SIG, T, 20_004, 37, dividend_yield=0.01, dividends=divs, model=model,
                                         option_type=opt, seed=5)
            p = _ffi.make_params(model=model.lower(), is_put=(opt == "put"), semantics="two_pass", n_paths=20_004, n_steps=37,
                                 S0=S0, K=K, r=R, sigma=SIG, T=T, seed=5, v0=SIG ** 2, kappa=2.0, theta=SIG ** 2, xi=0.3, rho=-0.7)
            o = ctx.price_american_div(p, 0.01, divs)
            assert isinstance(r, DividendResult) and float(r) == r.price == o["price"]
            assert (r.n_exercised, r.sum_nitm, r.n_paths, r.folded, r.dividend_steps) == (o["n_exercised"], o["sum_nitm"], 20_004, False, 3)
            assert r.stderr == math.sqrt(max(o["sumsq"] / 20_004 - o["price"] ** 2, 0.0) / 20_004)
            assert r.info["first_dividend_step"] == o["first_div_step"] == 8
    y = price_american_dividends(S0, K, R, SIG, T, 131_072, 12, dividend_yield=0.03)
    assert y.folded and y.dividend_steps == 0


def test_invalid_arguments_raise(ctx):
    from options_model_amd import price_american_dividends
    p = params(M=4096, N=20)
    for q, divs in ((math.nan, []), (0.0, [(0.0, 1.0)]), (0.0, [(1.5, 1.0)]), (0.0, [(0.5, -1.0)]), (0.0, [(0.5, math.inf)]),
                    (0.0, [(0.5, 1.0, "proportional")]), (0.0, [(0.5, 0.1, 5)])):
        with pytest.raises(_ffi.OmcError):
            ctx.price_american_div(p, q, divs)
    for bad in (params(M=4096, N=20, antithetic=False), _ffi.make_params(semantics="reference", n_paths=4096, n_steps=20)):
        with pytest.raises((_ffi.OmcError, ValueError)):
            ctx.price_american_div(bad, 0.0, [(0.5, 1.0)])
    keep = ctx.empty((21, 4000), np.float32)
    with pytest.raises(ValueError):  # -6: leading dimension below n_paths
        ctx.price_american_div(p, 0.0, [(0.5, 1.0)], S_keep=keep)
    keep.free()
    assert ctx.price_american_div(p, 0.0, [(0.5, 1.0)])["n_div_steps"] == 1  # and the context still prices
    for kw in (dict(dividend_yield=math.inf), dict(dividends=[(0.5, 1.0, "scrip")]), dict(dividends=[(0.5,)]),
               dict(dividends=[(2.0, 1.0)]), dict(dividends=[(0.5, 1.0, "proportional")]), dict(model="sabr"),
               dict(option_type="straddle")):
        with pytest.raises((_ffi.OmcError, ValueError)):
            price_american_dividends(S0, K, R, SIG, T, 4096, 20, **kw)


def test_distributed_context_is_refused(ctx):
    c = _ffi.Context(0)
    try:
        p = params(M=4096, N=20)
        before = flat(c.price_american_div(p, 0.0, [(0.5, 1.0)]))
        c.set_allreduce_hook(lambda dptr, count: None)
        out = _ffi.DivResult()
        import ctypes as C
        assert c.lib.omc_price_american_div(c.handle, C.byref(p), 0.01, None, 0, C.byref(out), None, 0) == -10
        with pytest.raises(ValueError):
            c.price_american_div(p, 0.0, [(0.5, 1.0)])
        c.set_allreduce_hook(None)
        assert not diff(flat(c.price_american_div(p, 0.0, [(0.5, 1.0)])), before)
    finally:
        c.close()

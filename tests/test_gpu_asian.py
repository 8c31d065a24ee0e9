"""Asian (average-price) options on the multi-asset index: kinds OMC_BASKET_ASIAN_ARITHMETIC (5) and _GEOMETRIC (6) of
omc_price_american_basket, omc_price_american_basket_bounds and omc_price_american_basket_bounds_runnerup (DESIGN.md section
23; options_model_amd/csrc/omc_basket.hip, omc_basket_bounds.hip, omc_asian_bounds.hip, omc_asian_dev.h).

  1. the index matrix   the arithmetic kind against the float32 restatement of tests/helpers/asian_ref.py on the device's own asset
                        matrices, bit for bit, at every store width; the geometric kind against the float64 one within GEO_RTOL
  2. the pricing        omc_lsm_poly semantics 2 on the kept index matrix, bit for bit
  3. bounds, index      the numpy restatement on rebuilt outer states and inner paths; the European known answer
  4. bounds, index+spot the restatement, the fit, a table without spot terms against 3.'s call, what the spot buys
  5. determinism, refusals, the facade and the C example
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import asian_ref as ar
from helpers import basket_bounds_case as bc
from helpers import bounds_ref as br
from helpers import runnerup_ref as rr
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R = 100.0, 0.05
RHO3 = bc.RHO3
KEYS = ("price", "sum", "sumsq", "std", "zero_prob", "n_paths", "n_exercised", "n_zero", "sum_nitm", "folded")
# The geometric kind against float64: the worst relative error measured on an MI355X at the shapes below was 1.054e-6 (N = 7 and 9, d = 1
# and 3) and 4.490e-6 (N = 252, 4096 paths); the bound is 4 x the larger.  The error is the float32 rounding of the running
# log2 sum (up to 252 terms near 6.6, ulp 1.2e-4 at 1700) divided by t, then one exp2: a wrong rule is percent off.
GEO_RTOL = 4 * 4.490e-6


def _params(is_put=True, N=8, M=4096, stream=0, T=1.0, seed=42, pair_offset=0):
    return _ffi.make_params(model="gbm", is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N, S0=100.0, K=K, r=R,
                            sigma=0.2, T=T, seed=seed, stream=stream, pair_offset=pair_offset)


def _basket(d, kind):
    """d = 1: one asset whose weight is not 1 (the basket value is a rounded product); d = 3: unequal everything"""
    if d == 1:
        return _ffi.make_basket([104.0], [0.27], [0.02], [0.95], None, kind)
    return _ffi.make_basket([100.0, 95.0, 105.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03], [0.5, 0.3, 0.2], RHO3, kind)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _priced(ctx, p, b, pad=0):
    d, ld = int(b.n_assets), p.n_paths + pad
    keep = ctx.empty((p.n_steps + 1, ld), np.float32)
    akeep = ctx.empty((d, p.n_steps + 1, ld), np.float32)
    out = ctx.price_american_basket(p, b, S_keep=keep, assets_keep=akeep)
    ref = ctx.lsm_poly(keep, p.K, p.r, p.T, bool(p.is_put), "two_pass", n_paths=p.n_paths)
    S, A = keep.to_host()[:, :p.n_paths], akeep.to_host()[:, :, :p.n_paths]
    keep.free()
    akeep.free()
    return out, ref, S, A


# ------------------------------------------------------------------ 1. the index matrix
@pytest.mark.parametrize("vec", [1, 2, 4])
@pytest.mark.parametrize("N", [7, 9])  # neither a multiple of the four-step Philox block
@pytest.mark.parametrize("d", [1, 3])
def test_arithmetic_index_is_the_restatement_bit_for_bit(ctx, d, N, vec):
    ctx.set_option("gbm_vec", vec)
    try:
        for is_put in (True, False):
            p = _params(is_put=is_put, N=N, stream=3, pair_offset=1234 if is_put else 0)
            b = _basket(d, "asian")
            out, ref, S, A = _priced(ctx, p, b)
            X, B, _ = ar.arithmetic_index(A, ar.weights(b))
            np.testing.assert_array_equal(_bits(S), _bits(X))
            np.testing.assert_array_equal(_bits(S[0]), _bits(B[0]))  # row 0 is B_0
            assert out["index0"] == _ffi.basket_table(p, b)[3] and (out["kind"], out["n_assets"]) == (5, d)
            assert abs(float(S[0, 0]) / out["index0"] - 1.0) <= 2.0 ** -22
            # the assets are the plain basket's: the kind touches the index alone
            _, _, S0, A0 = _priced(ctx, p, ar.as_kind(b, "basket"))
            np.testing.assert_array_equal(_bits(A), _bits(A0))
            np.testing.assert_array_equal(_bits(B), _bits(S0))
            assert [out[k] for k in KEYS] == [ref[k] for k in KEYS]  # 2. the pricing
    finally:
        ctx.set_option("gbm_vec", 0)


def test_an_odd_leading_dimension_takes_scalar_stores(ctx):
    p, b = _params(N=9, M=1026, stream=2), _basket(3, "asian")
    _, _, S, A = _priced(ctx, p, b, pad=3)
    np.testing.assert_array_equal(_bits(S), _bits(ar.arithmetic_index(A, ar.weights(b))[0]))


@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("d", [1, 3])
def test_one_date_is_the_plain_basket(ctx, d, kind):
    p = _params(N=1, stream=1)
    out, ref, S, A = _priced(ctx, p, _basket(d, kind))
    out0, _, S0, A0 = _priced(ctx, p, _basket(d, "basket"))
    if kind == "asian":
        np.testing.assert_array_equal(_bits(S), _bits(S0))
        assert [out[k] for k in KEYS] == [out0[k] for k in KEYS]
    else:
        np.testing.assert_allclose(S, S0, rtol=GEO_RTOL)
    np.testing.assert_array_equal(_bits(A), _bits(A0))


@pytest.mark.parametrize("d,N,M", [(1, 7, 4096), (3, 7, 4096), (1, 9, 4096), (3, 9, 4096), (1, 252, 4096), (3, 252, 4096)])
def test_geometric_index_against_float64(ctx, d, N, M):
    worst = 0.0
    for is_put in (True, False):
        p, b = _params(is_put=is_put, N=N, M=M, stream=4), _basket(d, "asian-geometric")
        out, ref, S, A = _priced(ctx, p, b)
        X = ar.geometric_index(A, ar.weights(b))
        np.testing.assert_array_equal(_bits(S[0]), _bits(ar.basket_value(A[:, 0], ar.weights(b))))  # row 0 is B_0
        worst = max(worst, float(np.abs(S / X - 1.0).max()))
        assert (out["kind"], out["n_assets"]) == (6, d)
        assert [out[k] for k in KEYS] == [ref[k] for k in KEYS]  # 2. the pricing
        Xa = ar.arithmetic_index(A, ar.weights(b))[0]
        assert (Xa[1:] >= S[1:] * (1.0 - 2 * GEO_RTOL)).all()  # the arithmetic average is at least the geometric one
    print(f"geometric, d {d}, N {N}: worst relative error {worst:.3e} (bound {GEO_RTOL:.3e})")
    assert worst <= GEO_RTOL


# ------------------------------------------------------------------ 3. bounds with the policy on the average alone
SIZES = dict(n_lower=4096, n_outer=64, n_inner=192)  # 96 inner pairs on 64 lanes: the refill
N_SMALL = 7
CASES = {"d1-put": (1, True), "d3-call": (3, False)}


@pytest.fixture(scope="module", params=list(CASES))
def spots(request, ctx):
    """the device's own lower, outer and inner spots of a case, shared by the policies that are checked on them (the inner
    items are rebuilt once and kept)"""
    d, is_put = CASES[request.param]
    p, b = _params(is_put=is_put, N=N_SMALL, stream=6), _basket(d, "asian")
    sp = ar.device_spots(ctx, p, b, **SIZES)
    cache = {}
    raw = sp["inner"]

    def inner(i, t):
        if (i, t) not in cache:
            cache[(i, t)] = raw(i, t)
        return cache[(i, t)]

    sp["inner"] = inner
    yield p, b, sp
    sp["free"]()


@pytest.mark.parametrize("policy", ["textbook", "given"])
def test_index_bounds_equal_restatement(ctx, spots, policy):
    p, b, sp = spots
    given = ar.given_table4(ctx, p, b) if policy == "given" else None
    dev = ctx.price_american_basket_bounds(p, b, policy=policy, betas=given, want_q=True, want_samples=True, **SIZES)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    else:
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, b, policy))
    lo, up = ar.check_against_restatement(ctx, p, b, dev, regressors="index", sp=sp, **SIZES)
    assert (dev["kind"], dev["n_assets"]) == (5, int(b.n_assets)) and dev["index0"] == _ffi.basket_table(p, b)[3]
    assert lo["n_exercised"] < SIZES["n_lower"] and (lo["n_exercised"] > 0 or not p.is_put)  # the put is exercised early
    # three inner items from their stored (S_t, c_t), one of them at t = 0 where the state is 0
    N = N_SMALL
    assert not sp["Co"][0].any()
    for i, t in ((0, 0), (5, 3), (63, N - 1)):
        X, _ = sp["inner"](i, t)
        assert (_bits(X[0]) == _bits(sp["Xo"][t, i])).all()  # the item starts at the outer state
        tau, Z, ties = br.first_stop(X, t, N, K, p.r, p.T, bool(p.is_put), dev["betas"])
        assert ties == 0
        np.testing.assert_allclose(dev["q"][i, t], Z.sum() / Z.size, rtol=1e-12, atol=1e-12 * K)
    # an inner path continues the average, it does not restart it: from c = 0 the item's first index would be B, not X
    X, B = sp["inner"](5, 3)
    assert not np.array_equal(_bits(X[1]), _bits(B[1]))


@pytest.mark.parametrize("is_put", [True, False])
def test_european_geometric_known_answer(ctx, is_put):
    """the geometric kind, one asset, a table that never exercises: the lower bound is the European geometric-average option"""
    N, S0, sig, q = 12, 100.0, 0.3, 0.02
    p = _params(is_put=is_put, N=N)
    kw = dict(policy="given", betas=np.zeros((N + 1, 4)), n_lower=400_000, n_outer=64, n_inner=64)
    g = ctx.price_american_basket_bounds(p, _ffi.make_basket([S0], [sig], [q], [1.0], None, "asian-geometric"), **kw)
    cf = ar.geometric_asian_european(S0, K, R, q, sig, 1.0, N, is_put)
    print(f"put {is_put}: lower {g['lower']:.5f} ({g['se_lower']:.5f})  closed form {cf:.5f}")
    assert g["n_exercised_lower"] == 0 and g["inner_path_steps"] == 64 * 64 * N * (N + 1) // 2
    assert abs(g["lower"] - cf) <= 4 * g["se_lower"]
    if not is_put:  # the arithmetic average is at least the geometric one, path by path
        a = ctx.price_american_basket_bounds(p, _ffi.make_basket([S0], [sig], [q], [1.0], None, "asian"), **kw)
        assert a["lower"] >= g["lower"] - 4 * math.hypot(a["se_lower"], g["se_lower"])
        assert a["lower"] > g["lower"]  # the same normals: AM >= GM on every path


# ------------------------------------------------------------------ 4. bounds with the policy on the average and the spot
@pytest.mark.parametrize("policy", ["textbook", "given"])
def test_index_spot_bounds_equal_restatement(ctx, spots, policy):
    p, b, sp = spots
    given = ar.given_table8(ctx, p, b) if policy == "given" else None
    dev = ctx.price_american_basket_bounds(p, b, policy=policy, betas=given, want_q=True, want_samples=True,
                                           regressors=ar.REG, **SIZES)
    assert dev["betas"].shape == (N_SMALL + 1, 8)
    if given is not None:
        np.testing.assert_array_equal(dev["betas"], given)
    else:  # the fit, date by date, on the device's own fitting paths
        _, _, X, B, _ = ar.paths(ctx, p, b)
        worst = rr.check_fit(X, B, K, p.r, p.T, bool(p.is_put), dev["betas"])
        print(f"fit: worst continuation difference / K {worst:.2e}")
        assert np.abs(dev["betas"][1:N_SMALL, 3:6]).max() > 0.0  # the spot terms are there
    ar.check_against_restatement(ctx, p, b, dev, regressors=ar.REG, sp=sp, **SIZES)
    assert (dev["kind"], dev["n_assets"]) == (5, int(b.n_assets))


@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("d,is_put", [(1, True), (3, False)])
def test_a_table_without_spot_terms_is_the_index_call(ctx, d, is_put, kind):
    p, b = _params(is_put=is_put, N=9, stream=7), _basket(d, kind)
    t4 = ar.given_table4(ctx, p, b)
    t8 = np.zeros((10, 8))
    t8[:, :3], t8[:, 6] = t4[:, :3], t4[:, 3]
    kw = dict(policy="given", want_q=True, want_samples=True, n_lower=4096, n_outer=64, n_inner=192)
    one = ctx.price_american_basket_bounds(p, b, betas=t4, **kw)
    two = ctx.price_american_basket_bounds(p, b, betas=t8, regressors=ar.REG, **kw)
    for k in ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_exercised_lower", "inner_path_steps", "index0",
              "n_assets", "kind"):
        assert one[k] == two[k], k
    np.testing.assert_array_equal(one["q"], two["q"])
    np.testing.assert_array_equal(one["samples"], two["samples"])
    np.testing.assert_array_equal(two["betas"], t8)
    assert 0 < one["n_exercised_lower"] < 4096


def test_what_the_spot_buys(ctx):
    """ATM put, sigma 0.4, ten dates: the policy that also sees the spot earns at least what the average alone earns, and
    stays below the upper bound, which holds for any policy.  Measured on an MI355X: index [8.3432 (0.0108), 9.2320
    (0.0329)], index+spot [9.0513 (0.0108), 9.0522 (0.0094)]: the lower bound rises by 0.7082, 46.3 combined standard errors,
    and the bracket all but closes."""
    p = _params(N=10, M=100_000)
    b = _ffi.make_basket([100.0], [0.4], [0.0], [1.0], None, "asian")
    kw = dict(policy="textbook", n_lower=400_000, n_outer=2048, n_inner=256)
    one = ctx.price_american_basket_bounds(p, b, **kw)
    two = ctx.price_american_basket_bounds(p, b, regressors=ar.REG, **kw)
    se = math.hypot(one["se_lower"], two["se_lower"])
    print(f"index      lower {one['lower']:.4f} ({one['se_lower']:.4f})  upper {one['upper']:.4f} ({one['se_upper']:.4f})")
    print(f"index+spot lower {two['lower']:.4f} ({two['se_lower']:.4f})  upper {two['upper']:.4f} ({two['se_upper']:.4f})")
    print(f"rise {two['lower'] - one['lower']:.4f} = {(two['lower'] - one['lower']) / se:.1f} combined standard errors")
    assert two["lower"] >= one["lower"] - 3 * se
    assert two["lower"] <= one["upper"] + 3 * one["se_upper"]
    assert two["lower"] <= two["upper"] + 3 * math.hypot(two["se_lower"], two["se_upper"])
    assert two["lower"] > one["lower"]  # measured at 46 combined standard errors, above the 4 that allow the assertion


# ------------------------------------------------------------------ 5. determinism, refusals, the facade, the C example
@pytest.mark.parametrize("kind", ar.KINDS)
def test_identical_calls_return_identical_bits(ctx, kind):
    p, b = _params(N=9, M=8192), _basket(3, kind)
    a = _priced(ctx, p, b)
    c = _priced(ctx, p, b)
    np.testing.assert_array_equal(_bits(a[2]), _bits(c[2]))
    assert [a[0][k] for k in KEYS] == [c[0][k] for k in KEYS]
    kw = dict(n_lower=4096, n_outer=64, n_inner=192, want_q=True, want_samples=True)
    for reg in ("index", ar.REG):
        x = ctx.price_american_basket_bounds(p, b, regressors=reg, **kw)
        ctx.price_american_basket_bounds(_params(N=5, M=2048), _basket(1, "best-of"), **kw)  # another call in between
        y = ctx.price_american_basket_bounds(p, b, regressors=reg, **kw)
        for k in ("lower", "se_lower", "upper", "se_upper", "n_exercised_lower", "inner_path_steps"):
            assert x[k] == y[k], (reg, k)
        for k in ("q", "samples", "betas"):
            np.testing.assert_array_equal(x[k], y[k])


def _rc_bounds(ctx, entry, p, b, policy=1, betas=None):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, 1000, 64, 64
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.BasketBounds()
    t = None if betas is None else np.ascontiguousarray(betas, np.float64)
    return getattr(ctx.lib, entry)(ctx.handle, C.byref(p), C.byref(b), C.byref(cfg), t.ctypes.data if t is not None else None,
                                   None, None, None, C.byref(out))


def test_refusals(ctx):
    p = _params()
    one, two = "omc_price_american_basket_bounds", "omc_price_american_basket_bounds_runnerup"
    for kind in ar.KINDS:
        b = _basket(3, kind)
        g = _ffi.BasketGreeks()
        assert ctx.lib.omc_price_american_basket_greeks(ctx.handle, C.byref(p), C.byref(b), 0.01, 1, None, None, C.byref(g)) == -32
        assert _rc_bounds(ctx, one, p, b) == 0 and _rc_bounds(ctx, two, p, b) == 0
        assert _rc_bounds(ctx, two, p, _basket(1, kind)) == 0  # one asset has a spot too
        assert _rc_bounds(ctx, two, p, b, policy=2) == -4 and _rc_bounds(ctx, two, p, b, policy=0) == -4
        assert _rc_bounds(ctx, two, _params(N=513), b) == -16
        assert _rc_bounds(ctx, one, p, b, policy=3) == -7
    for k in (4, 7, 9):
        b = bc.with_fields(_basket(3, "asian"), kind=k)
        g = _ffi.BasketGreeks()
        out = _ffi.BasketResult()
        assert ctx.lib.omc_price_american_basket(ctx.handle, C.byref(p), C.byref(b), C.byref(out), None, None, 0) == -32
        assert ctx.lib.omc_price_american_basket_greeks(ctx.handle, C.byref(p), C.byref(b), 0.01, 1, None, None, C.byref(g)) == -32
        assert _rc_bounds(ctx, one, p, b) == -32 and _rc_bounds(ctx, two, p, b) == -32
    # the other kinds keep their refusals
    assert _rc_bounds(ctx, two, p, _basket(3, "basket")) == -35 and _rc_bounds(ctx, two, p, _basket(1, "best-of")) == -35
    assert _rc_bounds(ctx, one, p, _basket(3, "geometric")) == -34 and _rc_bounds(ctx, two, p, _basket(3, "geometric")) == -34
    with pytest.raises(ValueError):
        ctx.price_american_basket_bounds(p, _basket(3, "basket"), regressors=ar.REG)
    with pytest.raises(ValueError):
        ctx.price_american_basket_bounds(p, _basket(3, "asian"), regressors=rr.REG)
    assert ctx.price_american_basket(p, _basket(3, "asian"))["price"] > 0.0  # the context still prices


FAC = dict(n_lower=50_000, n_outer=256, n_inner=128)


def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_basket, price_american_basket_bounds, price_asian_option

    S0, sig, q, w = [100.0, 95.0, 105.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03], [0.5, 0.3, 0.2]
    for kind in ar.KINDS:
        r = price_american_basket(S0, K, R, sig, 1.0, 20_004, 12, correlation=RHO3, weights=w, dividend_yields=q, kind=kind,
                                  seed=5)
        p = _ffi.make_params(is_put=True, semantics="two_pass", n_paths=20_004, n_steps=12, K=K, r=R, T=1.0, seed=5)
        o = ctx.price_american_basket(p, _ffi.make_basket(S0, sig, q, w, RHO3, kind))
        assert (r.price, r.n_exercised, r.kind, r.n_assets, r.index0) == (o["price"], o["n_exercised"], kind, 3, o["index0"])
        for reg in ("index", ar.REG):
            f = price_american_basket_bounds(S0, K, R, sig, 1.0, 20_000, 10, correlation=RHO3, weights=w, dividend_yields=q,
                                             kind=kind, stream=5, ctx=ctx, regressors=reg, **FAC)
            pp = _ffi.make_params(is_put=True, semantics="two_pass", n_paths=20_000, n_steps=10, S0=S0[0], K=K, r=R,
                                  sigma=sig[0], T=1.0, seed=42, stream=5)
            d = ctx.price_american_basket_bounds(pp, _ffi.make_basket(S0, sig, q, w, RHO3, kind), regressors=reg, **FAC)
            assert (f.lower, f.upper, f.se_lower, f.se_upper) == (d["lower"], d["upper"], d["se_lower"], d["se_upper"])
            np.testing.assert_array_equal(f.betas, d["betas"])
            assert (f.kind, f.n_assets, f.regressors, f.betas.shape[1]) == (kind, 3, reg, 4 if reg == "index" else 8)
    # the thin one-asset call
    a = price_asian_option(100.0, K, R, 0.3, 1.0, 20_000, 12, option_type="call", averaging="geometric", dividend_yield=0.02,
                           seed=9)
    o = price_american_basket([100.0], K, R, [0.3], 1.0, 20_000, 12, weights=[1.0], dividend_yields=[0.02],
                              kind="asian-geometric", option_type="call", seed=9)
    assert (a.price, a.kind, a.n_assets, a.option_type) == (o.price, "asian-geometric", 1, "call")
    fb = price_asian_option(100.0, K, R, 0.3, 1.0, 20_000, 10, bounds=True, regressors=ar.REG, ctx=ctx, **FAC)
    db = price_american_basket_bounds([100.0], K, R, [0.3], 1.0, 20_000, 10, weights=[1.0], kind="asian", ctx=ctx,
                                      regressors=ar.REG, **FAC)
    assert (fb.lower, fb.upper, fb.kind, fb.regressors) == (db.lower, db.upper, "asian", ar.REG)
    assert fb.lower - 3 * fb.se_lower <= fb.upper + 3 * fb.se_upper


def test_c_example_prints_the_prices_and_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_asian"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_asian.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "100000", "12", "100000", "512", "128"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    p = _ffi.make_params(is_put=True, semantics="two_pass", n_paths=100_000, n_steps=12, S0=100.0, K=100.0, r=0.05, sigma=0.3,
                         T=1.0, seed=42)
    for name, kind in (("arithmetic", "asian"), ("geometric", "asian-geometric")):
        b = _ffi.make_basket([100.0], [0.3], [0.0], [1.0], None, kind)
        price = float(re.search(name + r" average put: price ([0-9.]+)", out).group(1))
        assert abs(price - ctx.price_american_basket(p, b)["price"]) < 1e-6, out
    b = _ffi.make_basket([100.0], [0.3], [0.0], [1.0], None, "asian")
    for name, reg in (("average alone", "index"), ("average and spot", ar.REG)):
        ref = ctx.price_american_basket_bounds(p, b, n_lower=100_000, n_outer=512, n_inner=128, regressors=reg)
        lo, up = (float(v) for v in re.search(name + r" *: bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
    assert "Greeks: refused (-32)" in out

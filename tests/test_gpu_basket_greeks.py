"""Frozen-policy pathwise Greeks of the multi-asset options (omc_price_american_basket_greeks,
options_model_amd/csrc/omc_basket_greeks.hip).

What is compared, and how tightly:
  * the device against the numpy restatement    tests/helpers/basket_greeks_ref.py on the device's OWN asset and index
                                                matrices (omc_price_american_basket's S_keep / assets_keep) with the policy
                                                the call returned: counts of every chain identical, values rel 1e-9 / abs
                                                1e-12, standard errors rel 1e-6 (helpers/basket_greeks_case.agrees)
  * base                                        omc_price_american_basket's: counts identical, price rel 1e-12
  * one asset of weight 1, no yield             omc_price_american_greeks on full storage, to the same tolerance
  * want_gamma = 0                              the bits of want_gamma = 1 in every field that is not gamma or up / down
  * the European policy, geometric index        central differences of e^{r dt} BSM(G0, sigma_G, q_G) (the library values at
                                                t = dt, as tests/test_gpu_greeks.py states it): within 4 standard errors
  * price_up / price_down                       omc_lsm_apply_frozen on the index matrix generated at S0_i (1 +- h): rel 1e-5
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import basket_greeks_case as gc
from helpers import dividend_ref as dr
from helpers.call_catalogue import diff, flat
from helpers.greeks_check import close
from options_model_amd import _ffi
from test_gpu_basket import CASE3, CASE8, KINDS, basket_of
from test_gpu_dividends import K, R, SHAPES, T, params

pytestmark = pytest.mark.gpu

SHAPES5 = SHAPES[:3] + [(4_096, 8), (4_096, 2)]
CASE2 = tuple(x[:2] for x in CASE3[:5]) + (np.array([[1.0, 0.5], [0.5, 1.0]]),)
LAWS = {2: CASE2, 3: CASE3, 8: CASE8}
H = 0.01


@pytest.fixture
def fold_opt(ctx):
    yield ctx
    ctx.set_option("fold_antithetic", 1)


# ------------------------------------------------------------------ 1. the device against the restatement
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [2, 3, 8])
@pytest.mark.parametrize("M,N", SHAPES5)
def test_device_equals_restatement(ctx, M, N, d, kind):
    b, _ = basket_of(LAWS[d], kind)
    for is_put, stream, off in ((True, 2, 4321), (False, 3, (1 << 33) + 5)):
        # seed 77: the restatement counts no decision within 1e-10 K of the continuation value in any of these cases
        # (asserted below), so the values of every case are compared
        p = params(is_put=is_put, M=M, N=N, seed=77, stream=stream, pair_offset=off)
        dev = ctx.price_american_basket_greeks(p, b, bump=H, want_betas=True)
        ref = gc.reference(ctx, p, b, dev["betas"], H)
        assert ref["ties"] == [0, 0, 0], (kind, is_put, ref["ties"])
        assert gc.agrees(dev, ref, d), (kind, is_put)
        assert (dev["n_assets"], dev["gamma_on"], dev["bump"], dev["ms_pass2"]) == (d, 1, H, 0.0)


# ------------------------------------------------------------------ 2. base is the pricing
@pytest.mark.parametrize("kind", KINDS)
def test_base_is_the_basket_pricing(ctx, kind):
    for case, (M, N) in ((CASE3, SHAPES5[0]), (CASE8, SHAPES5[1]), (CASE3, SHAPES5[4])):
        b, _ = basket_of(case, kind)
        for is_put in (True, False):
            p = params(is_put=is_put, M=M, N=N, seed=11, stream=4, pair_offset=99)
            g = ctx.price_american_basket_greeks(p, b, gamma=False)
            a = ctx.price_american_basket(p, b)
            for k in ("n_paths", "n_exercised", "n_zero", "sum_nitm", "folded", "n_assets", "kind", "index0"):
                assert g[k] == a[k], (k, g[k], a[k])
            assert close(g["price"], a["price"], rel=1e-12), (g["price"], a["price"])


# ------------------------------------------------------------------ 3. one asset: the single-asset Greeks
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,N", [SHAPES5[0], SHAPES5[2], SHAPES5[4]])
def test_one_asset_is_the_single_asset_greeks(fold_opt, M, N, kind):
    ctx = fold_opt
    ctx.set_option("fold_antithetic", 0)
    S0, sig = 93.0, 0.27
    for is_put in (True, False):
        p = params(is_put=is_put, M=M, N=N, seed=9, stream=1, pair_offset=12345, S0=S0, sigma=sig)
        g = ctx.price_american_basket_greeks(p, _ffi.make_basket([S0], [sig], [0.0], [1.0], kind=kind), bump=H)
        v = ctx.price_american_greeks(p, bump=H)
        assert v["folded"] == 0
        for k in ("n_exercised", "n_zero", "sum_nitm", "n_paths"):
            assert g[k] == v[k], k
        assert (g["n_exercised_up"], g["n_exercised_down"]) == ([v["n_exercised_up"]], [v["n_exercised_down"]])
        for k in ("price", "rho", "theta"):
            assert close(g[k], v[k]), (k, g[k], v[k])
        for k in ("delta", "gamma", "vega", "price_up", "price_down"):
            assert close(g[k][0], v[k]), (k, g[k], v[k])


# ------------------------------------------------------------------ 4. the gamma switch
@pytest.mark.parametrize("d", [1, 3, 8])
def test_without_gamma_the_other_fields_keep_their_bits(ctx, d):
    M, N = SHAPES5[1]
    for kind in KINDS:
        S0, sig, q, w_sum, w_max, rho = CASE8
        w = w_sum if kind in ("basket", "geometric") else w_max
        b = _ffi.make_basket(S0[:d], sig[:d], q[:d], w[:d], np.asarray(rho)[:d, :d], kind)
        p = params(M=M, N=N, seed=3, stream=7)
        on = ctx.price_american_basket_greeks(p, b, bump=0.02, gamma=True, want_betas=True)
        off = ctx.price_american_basket_greeks(p, b, bump=0.02, gamma=False, want_betas=True)
        assert (on["gamma_on"], off["gamma_on"]) == (1, 0)
        scen = ("gamma", "se_gamma", "price_up", "price_down", "n_exercised_up", "n_exercised_down", "gamma_on")
        assert gc.strip({k: v for k, v in on.items() if k not in scen}) == gc.strip({k: v for k, v in off.items() if k not in scen})
        for k in scen[:4]:
            assert len(off[k]) == d and all(math.isnan(x) for x in off[k]), k
        assert off["n_exercised_up"] == off["n_exercised_down"] == [0] * d


# ------------------------------------------------------------------ 5. European Greeks of the geometric index
@pytest.mark.parametrize("is_put", [True, False])
def test_european_policy_geometric_index_is_black_scholes(ctx, is_put):
    """All-n = 0 table: the price is e^{r dt} BSM(G0, sigma_G, q_G) (valued at t = dt), and the per-asset deltas and
    vegas, rho and theta are its derivatives: central differences through omc_basket_table."""
    M, N = 200_000, 8
    S0, sig, q, w, _, rho = CASE3

    def value(S0=S0, sig=sig, r=R, T_=T):
        p = params(is_put=is_put, M=M, N=N, r=r, T=T_)
        G0, sG, qG = _ffi.basket_table(p, _ffi.make_basket(S0, sig, q, w, rho, "geometric"))[4]
        return math.exp(r * T_ / N) * dr.bsm(G0, K, r, qG, sG, T_, is_put)

    def bumped(v, i, e):
        return [x + (e if j == i else 0.0) for j, x in enumerate(v)]

    p = params(is_put=is_put, M=M, N=N, seed=7, stream=1)
    g = ctx.price_american_basket_greeks(p, _ffi.make_basket(S0, sig, q, w, rho, "geometric"), gamma=False,
                                         betas=np.zeros((N + 1, 4)))
    assert g["n_exercised"] == 0 and g["sum_nitm"] == 0
    assert abs(g["price"] - value()) <= 4 * math.sqrt(max(g["sumsq"] / M - g["price"] ** 2, 0) / M)
    for i in range(3):
        want = (value(S0=bumped(S0, i, 0.01)) - value(S0=bumped(S0, i, -0.01))) / 0.02
        assert abs(g["delta"][i] - want) <= 4 * g["se_delta"][i], ("delta", i, g["delta"][i], want, g["se_delta"][i])
        want = (value(sig=bumped(sig, i, 1e-4)) - value(sig=bumped(sig, i, -1e-4))) / 2e-4
        assert abs(g["vega"][i] - want) <= 4 * g["se_vega"][i], ("vega", i, g["vega"][i], want, g["se_vega"][i])
    want = (value(r=R + 1e-5) - value(r=R - 1e-5)) / 2e-5
    assert abs(g["rho"] - want) <= 4 * g["se_rho"], ("rho", g["rho"], want, g["se_rho"])
    want = -(value(T_=T + 1e-4) - value(T_=T - 1e-4)) / 2e-4
    assert abs(g["theta"] - want) <= 4 * g["se_theta"], ("theta", g["theta"], want, g["se_theta"])


# ------------------------------------------------------------------ 6. the scenario prices are regenerated pricings
@pytest.mark.parametrize("d,kind", [(2, "best-of"), (3, "basket")])
def test_scenario_prices_are_the_pricings_at_the_bumped_spots(ctx, d, kind):
    """(200,000 x 40, the size tests/test_gpu_greeks.py states the 1e-5 at: the regenerated float32 paths round differently,
    and ONE path near the boundary that decides the other way moves a 20,000-path price by more than that)"""
    M, N = 200_000, 40
    b, _ = basket_of(LAWS[d], kind)
    p = params(M=M, N=N, seed=31, stream=2)
    g = ctx.price_american_basket_greeks(p, b, bump=H, want_betas=True)
    keep = ctx.empty((N + 1, M), np.float32)
    for i in range(d):
        for lam, key in ((1.0 + H, "price_up"), (1.0 - H, "price_down")):
            bb = gc.with_fields(b)
            bb.S0[i] = b.S0[i] * lam
            ctx.price_american_basket(p, bb, S_keep=keep)
            ref = ctx.lsm_apply_frozen(keep, p.K, p.r, p.T, True, g["betas"], want_state=False)
            assert close(g[key][i], ref["price"], rel=1e-5), (key, i, g[key][i], ref["price"])
    keep.free()


# ------------------------------------------------------------------ 7. given tables
def test_given_tables_with_holes_and_feeding_the_policy_back(ctx):
    M, N = 20_008, 31
    for d, kind, is_put in ((3, "worst-of", True), (8, "basket", False), (2, "geometric", True)):
        b, _ = basket_of(LAWS[d], kind)
        p = params(is_put=is_put, M=M, N=N, seed=13, stream=5)
        fitted = ctx.price_american_basket_greeks(p, b, bump=H, want_betas=True)
        again = ctx.price_american_basket_greeks(p, b, bump=H, betas=fitted["betas"], want_betas=True)
        assert again["sum_nitm"] == 0 and fitted["sum_nitm"] > 0
        assert gc.strip({k: v for k, v in fitted.items() if k != "sum_nitm"}) == \
            gc.strip({k: v for k, v in again.items() if k != "sum_nitm"})
        table = fitted["betas"].copy()
        table[np.arange(N + 1) % 3 == 1, 3] = 0.0  # holes: no exercise on those dates
        dev = ctx.price_american_basket_greeks(p, b, bump=H, betas=table, want_betas=True)
        np.testing.assert_array_equal(dev["betas"], table)
        ref = gc.reference(ctx, p, b, table, H)
        assert ref["ties"] == [0, 0, 0] and gc.agrees(dev, ref, d)
        assert dev["n_exercised"] <= fitted["n_exercised"]  # fewer dates to fire on


# ------------------------------------------------------------------ 8. determinism
def test_two_calls_return_identical_bits(ctx):
    b, _ = basket_of(CASE8, "best-of")
    p = params(M=20_002, N=50, seed=42, stream=3)
    a0 = ctx.price_american_basket(p, b)
    g1 = ctx.price_american_basket_greeks(p, b, want_betas=True)
    a1 = ctx.price_american_basket(p, b)
    g2 = ctx.price_american_basket_greeks(p, b, want_betas=True)
    assert gc.strip(g1) == gc.strip(g2) and gc.strip(a0) == gc.strip(a1)
    assert gc.strip(ctx.price_american_basket_greeks(params(M=20_002, N=50, seed=42, stream=3, is_put=False), b)) != gc.strip(g1)


# ------------------------------------------------------------------ 9. error codes
def test_error_codes_and_the_context_still_prices(ctx):
    lib = ctx.lib
    p = params(M=4096, N=20)
    good, _ = basket_of(CASE3, "basket")
    out = _ffi.BasketGreeks()
    before = flat(ctx.price_american_basket_greeks(p, good)), flat(ctx.price_american_basket(p, good))

    def call(q, b, bump, o, c=ctx):
        return c.lib.omc_price_american_basket_greeks(c.handle, C.byref(q) if q is not None else None,
                                                      C.byref(b) if b is not None else None, bump, 1, None, None, o)

    assert lib.omc_price_american_basket_greeks(None, C.byref(p), C.byref(good), H, 1, None, None, C.byref(out)) == -7
    assert call(p, good, H, None) == -7
    assert call(None, good, H, C.byref(out)) == -7
    assert call(params("heston", 0, M=4096, N=20), good, H, C.byref(out)) == -12
    assert call(p, None, H, C.byref(out)) == -29
    assert call(p, _ffi.make_basket([100.0, -1.0], [0.2, 0.2]), H, C.byref(out)) == -30
    assert call(p, _ffi.make_basket([100.0, 90.0], [0.2, 0.2], kind=9), H, C.byref(out)) == -32
    npd = [[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]]
    assert call(p, _ffi.make_basket([100.0] * 3, [0.2] * 3, correlation=npd), H, C.byref(out)) == -31
    assert call(params(M=4097, N=20), good, H, C.byref(out)) == -3
    assert call(params(M=4096, N=20, antithetic=False), good, H, C.byref(out)) == -24
    assert call(_ffi.make_params(semantics="reference", n_paths=4096, n_steps=20), good, H, C.byref(out)) == -11
    assert call(params(M=4096, N=20, pair_offset=(1 << 40) - 2047), good, H, C.byref(out)) == -33
    for bump in (0.0, 0.6, -0.01, float("nan")):
        assert call(p, good, bump, C.byref(out)) == -4
    assert b"bump" in lib.omc_last_error()
    assert call(p, good, 0.5, C.byref(out)) == 0
    with pytest.raises(ValueError):
        ctx.price_american_basket_greeks(p, good, betas=np.zeros((5, 4)))
    c2 = _ffi.Context(ctx.device)
    try:
        c2.set_allreduce_hook(lambda dptr, count: None)
        assert call(p, good, H, C.byref(out), c2) == -10
        c2.set_allreduce_hook(None)
        assert not diff(flat(c2.price_american_basket_greeks(p, good)), before[0])
    finally:
        c2.close()
    assert not diff(flat(ctx.price_american_basket_greeks(p, good)), before[0])
    assert not diff(flat(ctx.price_american_basket(p, good)), before[1])


# ------------------------------------------------------------------ 10. facade and example
def test_facade_returns_the_ffi_numbers(ctx):
    from options_model_amd import BasketGreeksResult, price_american_basket_greeks
    S0, sig, q, _, _, rho = CASE3
    for kind in KINDS:
        for opt in ("put", "call"):
            r = price_american_basket_greeks(S0, K, R, sig, T, 20_004, 37, correlation=rho, dividend_yields=q, kind=kind,
                                             option_type=opt, bump=0.02, seed=5)
            w = [1.0 / 3] * 3 if kind in ("basket", "geometric") else [1.0] * 3
            p = _ffi.make_params(is_put=(opt == "put"), semantics="two_pass", n_paths=20_004, n_steps=37, K=K, r=R, T=T, seed=5)
            o = ctx.price_american_basket_greeks(p, _ffi.make_basket(S0, sig, q, w, rho, kind), bump=0.02, want_betas=True)
            assert isinstance(r, BasketGreeksResult) and float(r) == r.price == o["price"]
            for k in ("delta", "gamma", "vega", "se_delta", "se_gamma", "se_vega", "price_up", "price_down", "rho", "theta",
                      "se_rho", "se_theta", "n_exercised", "index0", "bump"):
                assert getattr(r, k) == o[k], k
            assert (r.n_assets, r.kind, r.n_paths, r.info["weights"]) == (3, kind, 20_004, w)
            np.testing.assert_array_equal(r.betas, o["betas"])
    r = price_american_basket_greeks([100.0, 110.0], K, R, [0.2, 0.3], T, 4_096, 20, weights=[0.7, 0.2], gamma=False)
    p = _ffi.make_params(semantics="two_pass", n_paths=4_096, n_steps=20, K=K, r=R, T=T, seed=42)
    o = ctx.price_american_basket_greeks(p, _ffi.make_basket([100.0, 110.0], [0.2, 0.3], None, [0.7, 0.2]), gamma=False)
    assert r.delta == o["delta"] and all(math.isnan(x) for x in r.gamma)


def test_c_example_prints_the_same_greeks(tmp_path, ctx):
    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_basket_greeks"
    subprocess.run(["gcc", "-O2", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_basket_greeks.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "100000", "50"], check=True, capture_output=True, text=True).stdout
    b = _ffi.make_basket(*CASE3[:4], CASE3[5], "basket")
    p = _ffi.make_params(is_put=True, semantics="two_pass", n_paths=100000, n_steps=50, K=100.0, r=0.05, T=1.0, seed=42)
    g = ctx.price_american_basket_greeks(p, b, bump=0.01)
    assert abs(float(re.search(r"price ([-0-9.]+)", out).group(1)) - g["price"]) < 1e-6
    for i in range(3):
        m = re.search(rf"asset {i}: delta ([-0-9.eE+]+) .*gamma ([-0-9.eE+]+) .*vega ([-0-9.eE+]+)", out)
        for got, key in zip(m.groups(), ("delta", "gamma", "vega")):
            assert abs(float(got) - g[key][i]) <= 1e-6 * max(1.0, abs(g[key][i])), (i, key, got, g[key][i])
    m = re.search(r"rho ([-0-9.eE+]+) .*theta ([-0-9.eE+]+)", out)
    assert abs(float(m.group(1)) - g["rho"]) <= 1e-6 * abs(g["rho"]) + 1e-6
    assert abs(float(m.group(2)) - g["theta"]) <= 1e-6 * abs(g["theta"]) + 1e-6

"""Frozen-policy pathwise Greeks of the two-pass flow (omc_price_american_greeks, options_model_amd/csrc/omc_greeks.hip)
against the numpy restatement of their definitions (tests/helpers/greeks_ref.py) on the very matrix the device stores,
against omc_price_american, against Black-Scholes for the all-n = 0 (European) policy, and for determinism.  (Sweep 13 of
tests/test_gpu_fuzz.py runs the same comparison over random shapes: all four kernel variants, short and ragged matrices,
pair offsets, given policies with holes.)

Agreement with the restatement: exercise counts of the three scenarios identical -- unless the restatement shows at
least as many decisions taken within 1e-10 K of the continuation value (ties: either branch is worth the same, and the
restatement's non-fused arithmetic may take the other one) -- and every Greek, price_up and price_down to rel 1e-9."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import greeks_ref as gr
from helpers.greeks_check import agrees as _agrees
from helpers.greeks_check import close as _close
from helpers.greeks_check import stored as _stored
from oracle import cpu as orc
from options_model_amd import _ffi
from options_model_amd.pricer import BlackScholesGreeks as BSG

pytestmark = pytest.mark.gpu

HESTON = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)


@pytest.fixture
def fold_opt(ctx):
    yield ctx
    ctx.set_option("fold_antithetic", 1)


def _restate(ctx, p, d, h):
    S = _stored(ctx, p)
    Sh = S.to_host()
    S.free()
    return gr.greeks(Sh, p.K, p.r, p.T, p.is_put, d["betas"], p.S0, p.sigma, h=h, gbm=(p.model == 0))


FULL = [
    dict(model="gbm", is_put=True),
    dict(model="gbm", is_put=False, K=95.0),
    dict(model="gbm", is_put=True, antithetic=False, K=105.0),
    dict(model="gbm", is_put=False, antithetic=False, sigma=0.3),
    dict(model="heston", is_put=True, heston_scheme=0),
    dict(model="heston", is_put=False, heston_scheme=1),
    dict(model="heston", is_put=True, heston_scheme=2, K=110.0),
]


@pytest.mark.parametrize("case", FULL, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_full_storage_matches_restatement(fold_opt, case):
    ctx = fold_opt
    ctx.set_option("fold_antithetic", 0)
    kw = dict(semantics="two_pass", n_paths=30_000, n_steps=40, seed=21, stream=5)
    kw.update(HESTON if case["model"] == "heston" else {})
    kw.update(case)
    p = _ffi.make_params(**kw)
    d = ctx.price_american_greeks(p, bump=0.01, want_betas=True)
    assert d["folded"] == 0
    _agrees(d, _restate(ctx, p, d, 0.01), p)


@pytest.mark.parametrize("M,opt,is_put,K", [(40_000, 2, True, 100.0), (40_000, 2, False, 100.0),
                                            (65_536, 1, True, 100.0), (65_536, 1, True, 90.0)])
def test_folded_storage_matches_restatement(fold_opt, M, opt, is_put, K):
    ctx = fold_opt
    ctx.set_option("fold_antithetic", opt)
    p = _ffi.make_params(semantics="two_pass", is_put=is_put, K=K, n_paths=M, n_steps=40, seed=23, stream=6)
    d = ctx.price_american_greeks(p, bump=0.02, want_betas=True)
    assert d["folded"] == 1
    S = ctx.gbm_paths(M // 2, p.n_steps, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, antithetic=False).to_host()
    c0, g = orc.fold_constants(p.S0, p.K, p.r, p.sigma, p.T, p.n_steps)
    ref = gr.greeks(S, p.K, p.r, p.T, is_put, d["betas"], p.S0, p.sigma, h=0.02, cK=orc.fold_table(p.n_steps, c0, g))
    _agrees(d, ref, p)


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("is_put", [True, False])
def test_base_is_the_two_pass_pricing(fold_opt, fold, is_put):
    ctx = fold_opt
    ctx.set_option("fold_antithetic", fold)
    p = _ffi.make_params(semantics="two_pass", is_put=is_put, n_paths=100_000, n_steps=50, seed=42, stream=9)
    d = ctx.price_american_greeks(p, want_betas=True)
    a = ctx.price_american(p)
    assert d["folded"] == a["folded"] == fold
    for k in ("n_exercised", "n_zero", "sum_nitm", "n_paths"):
        assert d[k] == a[k], k
    assert _close(d["price"], a["price"], rel=1e-12)
    N = p.n_steps
    if fold:
        S = ctx.gbm_paths(p.n_paths // 2, N, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, antithetic=False).to_host()
        c0, g = orc.fold_constants(p.S0, p.K, p.r, p.sigma, p.T, N)
        ref = orc.lsm_two_pass_folded(S, p.K, p.r, p.T, is_put, c0, g)
        rel = 1e-9
    else:
        S = ctx.gbm_paths(p.n_paths, N, p.S0, p.r, p.sigma, p.T, p.seed, p.stream)
        ref = ctx.lsm_poly(S, p.K, p.r, p.T, is_put, "two_pass")
        S.free()
        rel = 1e-12
    b = d["betas"][1:N]
    assert np.array_equal(b[:, 3], ref["nitm"][1:N].astype(np.float64))
    scale = np.abs(ref["betas"][1:N]).max(axis=0)
    assert np.all(np.abs(b[:, :3] - ref["betas"][1:N]) <= rel * np.maximum(np.abs(ref["betas"][1:N]), 1e-3 * scale))


@pytest.mark.parametrize("is_put", [True, False])
def test_european_policy_is_black_scholes(ctx, is_put):
    """All-n = 0 table: valued at t = dt the price is e^{r dt} C_BS, and so are its derivatives (plus the dt terms)."""
    S0, K, r, sig, T, N, M, h = 100.0, 100.0, 0.05, 0.2, 1.0, 50, 1_000_000, 0.01
    p = _ffi.make_params(semantics="two_pass", is_put=is_put, antithetic=False, n_paths=M, n_steps=N, seed=7, stream=1)
    d = ctx.price_american_greeks(p, bump=h, betas=np.zeros((N + 1, 4)))
    assert d["n_exercised"] == d["n_exercised_up"] == d["n_exercised_down"] == 0 and d["sum_nitm"] == 0
    kind = "put" if is_put else "call"
    bs = BSG.greeks(S0, K, T, r, sig, kind)
    C_ = BSG.black_scholes_price(S0, K, T, r, sig, kind)
    dt = T / N
    e = math.exp(r * dt)
    want = dict(delta=e * bs["Delta"], gamma=e * bs["Gamma"], vega=e * bs["Vega"] * 100,
                rho=e * (dt * C_ + bs["Rho"] * 100), theta=e * (bs["Theta"] * 365 - r / N * C_))
    for k, v in want.items():
        slack = 2e-3 * abs(v) if k == "gamma" else 0.0  # the central difference's O(h^2)
        assert abs(d[k] - v) <= 4 * d["se_" + k] + slack, (k, d[k], v, d["se_" + k])
    assert abs(d["price"] - e * C_) <= 4 * math.sqrt(max(d["sumsq"] / M - d["price"] ** 2, 0) / M)


@pytest.mark.parametrize("model", ["gbm", "heston"])
def test_scenarios_are_the_regenerated_pricings(fold_opt, model):
    """price_up = the frozen pricing of paths generated at S0 (1 + h); with no exercise the pathwise delta is the
    scenarios' central difference (with exercise that difference also carries the decision-boundary term)."""
    ctx = fold_opt
    ctx.set_option("fold_antithetic", 0)
    h, M, N = 0.01, 200_000, 40
    kw = dict(model=model, semantics="two_pass", is_put=True, n_paths=M, n_steps=N, seed=31, stream=2)
    kw.update(HESTON if model == "heston" else {})
    p = _ffi.make_params(**kw)
    d = ctx.price_american_greeks(p, bump=h, want_betas=True)
    for lam, key in ((1 + h, "price_up"), (1 - h, "price_down")):
        if model == "gbm":
            Sb = ctx.gbm_paths(M, N, p.S0 * lam, p.r, p.sigma, p.T, p.seed, p.stream)
        else:
            Sb = ctx.heston_paths(M, N, p.S0 * lam, p.r, p.T, p.v0, p.kappa, p.theta, p.xi, p.rho, p.seed, p.stream,
                                  scheme=p.heston_scheme)
        ref = ctx.lsm_apply_frozen(Sb, p.K, p.r, p.T, True, d["betas"], want_state=False)
        Sb.free()
        assert _close(d[key], ref["price"], rel=1e-5), (key, d[key], ref["price"])
    e = ctx.price_american_greeks(p, bump=h, betas=np.zeros((N + 1, 4)))
    fd = (e["price_up"] - e["price_down"]) / (2 * h * p.S0)
    assert abs(e["delta"] - fd) <= 4 * e["se_delta"], (e["delta"], fd, e["se_delta"])


def test_deterministic_and_isolated(fold_opt):
    ctx = fold_opt
    p = _ffi.make_params(semantics="two_pass", n_paths=200_000, n_steps=50, seed=42, stream=3)
    strip = lambda d: {k: v for k, v in d.items() if not k.startswith("ms_") and k != "betas"}  # noqa: E731
    a0 = ctx.price_american(p)
    g1 = ctx.price_american_greeks(p)
    a1 = ctx.price_american(p)
    g2 = ctx.price_american_greeks(p)
    assert strip(g1) == strip(g2)
    assert strip(a0) == strip(a1)
    q = _ffi.make_params(semantics="two_pass", n_paths=200_000, n_steps=50, seed=42, stream=3, is_put=False)
    assert strip(ctx.price_american_greeks(q)) != strip(g1)


def test_error_codes(ctx):
    lib = ctx.lib
    p = _ffi.make_params(semantics="two_pass", n_paths=1000, n_steps=10)
    g = _ffi.Greeks()
    call = lambda q, bump, out: lib.omc_price_american_greeks(ctx.handle, C.byref(q), bump, None, None, out)  # noqa: E731
    assert call(_ffi.make_params(semantics="reference", n_paths=1000, n_steps=10), 0.01, C.byref(g)) == -4
    assert call(p, 0.0, C.byref(g)) == -4
    assert call(p, 0.6, C.byref(g)) == -4
    assert call(p, float("nan"), C.byref(g)) == -4
    assert call(p, 0.01, None) == -7
    assert call(p, 0.5, C.byref(g)) == 0
    c2 = _ffi.Context(ctx.device)
    try:
        c2.set_allreduce_hook(lambda dptr, count: None)
        assert c2.lib.omc_price_american_greeks(c2.handle, C.byref(p), 0.01, None, None, C.byref(g)) == -10
        assert "one GPU" in c2.lib.omc_last_error().decode()
    finally:
        c2.close()


def test_headline_size(ctx):
    p = _ffi.make_params(semantics="two_pass", n_paths=1_000_000, n_steps=252, seed=42)
    d = ctx.price_american_greeks(p)
    a = ctx.price_american(p)
    assert d["folded"] == 1 == a["folded"]
    for k in ("n_exercised", "n_zero", "sum_nitm"):
        assert d[k] == a[k], k
    assert _close(d["price"], a["price"], rel=1e-12)
    assert -1.0 < d["delta"] < 0.0 and d["gamma"] > 0.0 and d["vega"] > 0.0 and d["rho"] < 0.0
    assert d["ms_greeks"] > 0.0

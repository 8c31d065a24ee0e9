"""What omc_price_american_jump_greeks offers without a GPU: the symbol, the header and the ABI
version, the facade's argument checks, the catalogue on the stand-in library, the cases' coverage, and the restatement
(helpers/jump_greeks_ref.py) checked against itself and against Merton's series:
  * on float64 paths, with the exercise steps, the in-the-money indicator and the jump counts held fixed, every pathwise
    Greek is the central finite difference of the frozen price in its parameter;
  * with the European table on 2^18 paths x 8 steps from the C oracle's Philox, price and Greeks -- the score terms of
    dlambda and theta included -- lie within 4 standard errors of Merton's series and its central differences."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from helpers import call_catalogue as cat
from helpers import jump_greeks_case as gc
from helpers import jump_greeks_catalogue as gcat
from helpers import jump_greeks_ref as gr
from helpers import jump_ref as jr
from options_model_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_symbol_header_and_abi_version():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    names = ["omc_price_american_jump_greeks"]
    assert sorted(_ffi.JUMP_GREEKS_SIGNATURES) == names
    others = (set(_ffi.SIGNATURES) | set(_ffi.JUMP_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_BOUNDS_SIGNATURES)
              | set(_ffi.BARRIER_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_GREEKS_SIGNATURES) | set(_ffi.CHAIN_BOUNDS_SIGNATURES))
    assert not set(_ffi.JUMP_GREEKS_SIGNATURES) & others
    assert len(_ffi.JUMP_GREEKS_SIGNATURES[names[0]][1]) == 8
    assert len(getattr(lib, names[0]).argtypes) == 8  # exported and bound
    header = open(os.path.join(ROOT, "include", "omc_jump_greeks.h")).read()
    assert '#include "omc.h"' in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(omc_[a-z0-9_]+)\s*\(", code))) == names
    assert re.search(r"\bint omc_price_american_jump_greeks\(omc_ctx\* ctx, const omc_params\* p, const omc_jump\* j, double q, "
                     r"double bump,\s*const double\* betas, double\* betas_out, omc_jump_greeks\* out\);", header)
    assert re.search(r"#define OMC_ABI_VERSION 14\b", open(os.path.join(ROOT, "include", "omc.h")).read())
    # the struct is omc_greeks followed by twelve doubles and one int64
    assert ctypes.sizeof(_ffi.JumpGreeks) == ctypes.sizeof(_ffi.Greeks) + 13 * 8
    assert _ffi.JumpGreeks.epsilon.offset == ctypes.sizeof(_ffi.Greeks)
    assert [n for n, _ in _ffi.JumpGreeks._fields_] == re.findall(
        r"\b(g|epsilon|se_epsilon|dlambda|se_dlambda|dmu_j|se_dmu_j|dsigma_j|se_dsigma_j|theta_score|se_theta_score|kappa|"
        r"drift_rate|n_jumps)[,;]", code.split("typedef struct {")[1].split("}")[0])


@pytest.mark.parametrize("kw,match", [
    (dict(bump=0.0), "bump"), (dict(bump=0.6), "bump"), (dict(bump=float("nan")), "bump"),
    (dict(model="Heston", heston_scheme="milstein"), "heston_scheme"),
    (dict(jump_intensity=-1.0), "jump_intensity"), (dict(jump_intensity=float("nan")), "jump_intensity"),
    (dict(jump_vol=-0.1), "jump_vol"), (dict(jump_mean=float("inf")), "jump_mean"), (dict(jump_intensity=4.5), "n_steps"),
    (dict(dividend_yield=float("nan")), "dividend"), (dict(model="SABR"), "model"), (dict(option_type="straddle"), "option_type")],
    ids=["bump-0", "bump-large", "bump-nan", "scheme", "lambda-negative", "lambda-nan", "vol-negative", "mean-inf", "x-above-1",
         "yield", "model", "option-type"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_american_jump_greeks

    args = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, jump_intensity=1.0, jump_mean=-0.1,
                jump_vol=0.15, device=10 ** 6)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_american_jump_greeks(**args)


def test_facade_is_exported():
    import options_model_amd as oma

    assert callable(oma.price_american_jump_greeks)
    fields = set(oma.JumpGreeksResult.__dataclass_fields__)
    assert {"delta", "gamma", "vega", "rho", "theta", "epsilon", "dlambda", "dmu_j", "dsigma_j", "theta_score", "se_dlambda",
            "se_dmu_j", "se_dsigma_j", "se_theta_score", "price_up", "price_down", "n_exercised_up", "n_exercised_down", "betas",
            "n_jumps", "kappa", "drift_rate", "bump"} <= fields


def test_the_catalogue_calls_every_symbol_of_the_extension_header():
    used = gcat.symbols_used()
    assert set(_ffi.JUMP_GREEKS_SIGNATURES) == set().union(*used.values())  # exactly the new symbol
    for e in gcat.CATALOGUE:
        assert used[e.name] == {"omc_" + e.family}, (e.name, used[e.name])
        assert e.name == f"{e.family}/{e.name.split('/')[1]}/{e.cls}"
    assert len({e.name for e in gcat.CATALOGUE}) == len(gcat.CATALOGUE)
    for fam in gcat.FAMILIES:
        assert {e.cls for e in gcat.CATALOGUE if e.family == fam} == {"S", "M"}
    assert sorted(gcat.DRAWING) == gcat.FAMILIES and not set(gcat.FAMILIES) & set(cat.FAMILIES)


def test_the_catalogue_entries_follow_the_key_sweep():
    class ArgLib(cat.RecordingLib):
        def __init__(self):
            super().__init__()
            self.params = []

        def __getattr__(self, name):
            fn = super().__getattr__(name)

            def noting(*args):
                self.params += [a._obj for a in args if isinstance(getattr(a, "_obj", None), _ffi.Params)]
                return fn(*args)
            return noting

    for e in gcat.CATALOGUE:
        ctx = cat.recording_context()
        ctx.lib = ArgLib()
        try:
            with cat.drawing(0x9E3779B97F4A7C15, 0xDEADBEEF, (1 << 32) - 3):
                e.call(ctx)
        finally:
            ctx.handle = None
        assert ctx.lib.params, e.name
        for p in ctx.lib.params:
            assert p.seed == 0x9E3779B97F4A7C15 and p.pair_offset == (1 << 32) - 3 and 0 <= p.stream - 0xDEADBEEF < 16, e.name


def test_the_grid_covers_the_list():
    g = gc.grid()
    assert len({gc.case_id(c) for c in g}) == len(g) == len(gc.MODELS) * len(gc.STEPS)
    assert {(c["model"], c["N"]) for c in g} == {(m, n) for m in gc.MODELS for n in gc.STEPS}
    assert {c["pairs"] for c in g} == set(gc.PAIRS) and {c["is_put"] for c in g} == {True, False}
    assert {(c["x"], c["sizes"]) for c in g} == {(x, s) for x in gc.XS for s in gc.SIZES}
    assert {(c["model"], c["x"]) for c in g} == {(m, x) for m in gc.MODELS for x in gc.XS}
    assert {(c["pairs"], c["x"]) for c in g} == {(p, x) for p in gc.PAIRS for x in gc.XS}
    assert {(c["model"], c["is_put"]) for c in g} == {(m, s) for m in gc.MODELS for s in (True, False)}
    assert all(c["x"] <= 1.0 for c in g)


def test_fuzz_cases_are_deterministic_and_cover_the_space():
    a = gc.fuzz_cases(8)
    assert a == gc.fuzz_cases(8) and gc.fuzz_cases(9)[:8] == a
    assert {c["model"] for c in a} == set(gc.MODELS) and {c["is_put"] for c in gc.fuzz_cases(16)} == {True, False}
    assert all(100 <= c["pairs"] <= 1200 and 1 <= c["N"] <= 13 and 0.0 < c["x"] <= 1.0 for c in gc.fuzz_cases(64))
    assert {c["N"] for c in gc.fuzz_cases(200)} == set(range(1, 14))


def test_vectorised_draws_are_jump_ref_draws():
    from oracle import cpu as orc

    thr = jr.table(3.0, -0.1, 0.15, 0.05, 0.0, 1.0, 9)[0]
    a = jr.draws(orc.philox4x32_10, 70, 9, 0x123456789, 3, (1 << 32) - 5, thr)
    b = gr.draws(orc.philox_words, 70, 9, 0x123456789, 3, (1 << 32) - 5, thr)
    assert a[0].sum() > 50 and np.array_equal(a[0], b[0])
    np.testing.assert_allclose(b[1], a[1], rtol=1e-14, atol=0.0)


# ------------------------------------------------------------------ the restatement against itself
S0, K, R, Q, SIG, T, N, PAIRS = 100.0, 100.0, 0.05, 0.02, 0.25, 1.0, 7, 3000
LAM, MU, SJ = 3.0, -0.1, 0.15


def _policy():
    """exercise where the payoff exceeds 3 - 60 u: a put about 7.5 in the money, a call about 1.9"""
    b = np.zeros((N + 1, 4))
    b[1:N] = (3.0, -60.0, 0.0, 1.0)
    b[4, 3] = 0.0  # a date without a fit
    return b


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
def test_pathwise_greeks_are_the_derivatives_of_the_frozen_price(is_put):
    """Central differences with relative float64 bumps of 1e-5 (absolute for r, q and mu_j).  With the steps, the
    in-the-money indicator and the jump counts held fixed the price is analytic in every parameter: the truncation error
    delta^2 f''' / 6 is below 1e-9 relative and the rounding error 1e-16 V / delta below 1e-9 of a Greek: 1e-6 holds with
    room.  At fixed counts lambda acts through the compensated drift alone: the pathwise part of dlambda."""
    rng = np.random.default_rng(11)
    Z = rng.standard_normal((N, PAIRS))
    n = np.concatenate([np.zeros((1, PAIRS), np.int64), rng.poisson(LAM * T / N, (N, PAIRS))])
    zJ = np.where(n > 0, rng.standard_normal((N + 1, PAIRS)), 0.0)
    h = 0.01

    def paths(S0_=S0, r=R, q=Q, sig=SIG, T_=T, lam=LAM, mu=MU, sj=SJ):
        return gr.simulate(S0_, r, q, sig, T_, N, Z, n, zJ, lam, mu, sj)

    S = paths()
    out = gr.greeks((S, paths(S0 * (1 + h)), paths(S0 * (1 - h))), S0, K, R, Q, T, is_put, _policy(), h, LAM, MU, SJ, sigma=SIG,
                    Z=Z, n=n, zJ=zJ)
    tex = out["tex"][0]
    assert out["ties"] == [0, 0, 0] and 0.05 < (tex < N).mean() < 0.95 and out["n_jumps"] == n.sum() > PAIRS
    s_k = S[tex, np.arange(S.shape[1])]
    itm = (K - s_k if is_put else s_k - K) > 0.0

    def price(r=R, T_=T, **kw):
        return gr.frozen_price(paths(r=r, T_=T_, **kw), K, r, T_, is_put, tex, itm)

    assert abs(price() - out["price"]) <= 1e-12 * out["price"]
    for greek, arg, x, d in (("delta", "S0_", S0, 1e-5 * S0), ("vega", "sig", SIG, 1e-5 * SIG), ("rho", "r", R, 1e-5),
                             ("epsilon", "q", Q, 1e-5), ("dmu_j", "mu", MU, 1e-5), ("dsigma_j", "sj", SJ, 1e-5 * SJ),
                             ("dlambda_pathwise", "lam", LAM, 1e-5 * LAM)):
        want = (price(**{arg: x + d}) - price(**{arg: x - d})) / (2.0 * d)
        assert abs(out[greek] - want) <= 1e-6 * abs(want), (greek, out[greek], want)
    # theta without its score part is -d/dT of the frozen price at fixed counts
    want = -(price(T_=T + 1e-5) - price(T_=T - 1e-5)) / 2e-5
    assert abs((out["theta"] - out["theta_score"]) - want) <= 1e-6 * abs(want)
    assert math.isfinite(out["gamma"])


def test_without_jumps_the_jump_greeks_vanish():
    Z = np.random.default_rng(3).standard_normal((N, 500))
    n = np.zeros((N + 1, 500), np.int64)
    S = gr.simulate(S0, R, Q, SIG, T, N, Z, n, n * 0.0, 0.0, MU, SJ)
    out = gr.greeks((S, S * 1.01, S * 0.99), S0, K, R, Q, T, True, _policy(), 0.01, 0.0, MU, SJ, sigma=SIG, Z=Z, n=n, zJ=n * 0.0)
    assert out["dmu_j"] == 0.0 and out["dsigma_j"] == 0.0 and out["theta_score"] == 0.0 and math.isnan(out["dlambda"])


# ------------------------------------------------------------------ the European table against Merton's series
@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
def test_european_table_is_mertons_series(is_put):
    """2^18 paths x 8 steps, lambda = 2, T = 1, seed 42 -- the case and seed of the GPU twin
    (tests/test_gpu_jump_greeks.py), checked here first so that it cannot fail there by sampling alone."""
    ref = gc.euro_restatement(is_put)
    want = gc.euro_closed_form(is_put)
    assert ref["n_exercised"] == 0 and ref["n_jumps"] > 0
    for k in gc.EURO_NAMES:
        print("EUROPEAN", k, ref[k], want[k], ref["se_" + k], (ref[k] - want[k]) / ref["se_" + k])
        assert abs(ref[k] - want[k]) <= 4.0 * ref["se_" + k], (k, ref[k], want[k], ref["se_" + k])

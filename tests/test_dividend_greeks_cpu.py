"""What omc_price_american_div_greeks offers without a GPU: the symbol, the header and the ABI
version, the facade's argument checks, the catalogue on the stand-in library, and the restatement
(helpers/dividend_greeks_ref.py) checked against itself: on float64 paths, with the exercise steps held fixed, every tangent
Greek is the central finite difference of the frozen-decision price in its parameter."""
import math
import os
import re

import numpy as np
import pytest

from helpers import call_catalogue as cat
from helpers import dividend_greeks_case as gc
from helpers import dividend_greeks_catalogue as gcat
from helpers import dividend_greeks_ref as gr
from helpers import dividend_ref as dr
from options_model_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_symbol_header_and_abi_version():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    names = ["omc_price_american_div_greeks"]
    assert sorted(_ffi.DIVIDEND_GREEKS_SIGNATURES) == names
    others = (set(_ffi.SIGNATURES) | set(_ffi.JUMP_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_BOUNDS_SIGNATURES)
              | set(_ffi.BARRIER_BOUNDS_SIGNATURES))
    assert not set(_ffi.DIVIDEND_GREEKS_SIGNATURES) & others
    assert len(_ffi.DIVIDEND_GREEKS_SIGNATURES[names[0]][1]) == 9
    assert len(getattr(lib, names[0]).argtypes) == 9  # exported and bound
    header = open(os.path.join(ROOT, "include", "omc_dividend_greeks.h")).read()
    assert '#include "omc.h"' in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(omc_[a-z0-9_]+)\s*\(", code))) == names
    assert re.search(r"\bint omc_price_american_div_greeks\(omc_ctx\* ctx, const omc_params\* p, double q, "
                     r"const omc_dividend\* d, int n_div,\s*double bump, const double\* betas, double\* betas_out, "
                     r"omc_div_greeks\* out\);", header)
    assert re.search(r"#define OMC_ABI_VERSION 14\b", open(os.path.join(ROOT, "include", "omc.h")).read())
    # the struct is omc_greeks followed by two doubles and two int32
    import ctypes
    assert ctypes.sizeof(_ffi.DivGreeks) == ctypes.sizeof(_ffi.Greeks) + 24
    assert _ffi.DivGreeks.epsilon.offset == ctypes.sizeof(_ffi.Greeks)


@pytest.mark.parametrize("kw,match", [
    (dict(bump=0.0), "bump"), (dict(bump=0.6), "bump"), (dict(bump=float("nan")), "bump"),
    (dict(model="Heston", heston_scheme="milstein"), "heston_scheme"),
    (dict(dividends=[(0.5,)]), "a dividend is"), (dict(dividends=[(0.5, 1.0, "stock")]), "kind"),
    (dict(dividends=[(0.0, 1.0)]), "time"), (dict(dividends=[(1.5, 1.0)]), "time"), (dict(dividends=[(0.5, -1.0)]), "amount"),
    (dict(dividends=[(0.5, 1.0, "proportional")]), "proportional"), (dict(dividend_yield=float("nan")), "dividend"),
    (dict(model="SABR"), "model"), (dict(option_type="straddle"), "option_type")],
    ids=["bump-0", "bump-large", "bump-nan", "scheme", "item", "kind", "time-0", "time-late", "negative", "proportional-1",
         "yield", "model", "option-type"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_american_dividend_greeks

    args = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, dividends=[(0.4, 1.0)], device=10 ** 6)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_american_dividend_greeks(**args)


def test_facade_is_exported():
    import options_model_amd as oma

    assert callable(oma.price_american_dividend_greeks)
    fields = set(oma.DividendGreeksResult.__dataclass_fields__)
    assert {"delta", "gamma", "vega", "rho", "theta", "epsilon", "se_epsilon", "price_up", "price_down", "n_exercised_up",
            "n_exercised_down", "betas", "dividend_steps", "first_dividend_step", "bump"} <= fields


def test_the_catalogue_calls_every_symbol_of_the_extension_header():
    used = gcat.symbols_used()
    assert set(_ffi.DIVIDEND_GREEKS_SIGNATURES) <= set().union(*used.values())
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


def test_fuzz_cases_are_deterministic_and_cover_the_space():
    a = gc.fuzz_cases(24)
    assert a == gc.fuzz_cases(24) and gc.fuzz_cases(25)[:24] == a
    assert {c["model"] for c in a} == set(gc.MODELS) and {c["is_put"] for c in a} == {True, False}
    assert {len(c["divs"]) for c in gc.fuzz_cases(64)} == set(range(6))
    assert all(c["M"] % 2 == 0 and all(1 <= k <= c["N"] for k, _, _ in c["divs"]) for c in a)


# ------------------------------------------------------------------ the restatement against itself
S0, K, R, Q, SIG, T, N, PAIRS = 100.0, 100.0, 0.05, 0.02, 0.25, 1.0, 7, 3000


def _policy():
    """exercise where the payoff exceeds 3 - 60 u: a put about 7.5 in the money, a call about 1.9"""
    b = np.zeros((N + 1, 4))
    b[1:N] = (3.0, -60.0, 0.0, 1.0)
    b[4, 3] = 0.0  # a date without a fit
    return b


@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
@pytest.mark.parametrize("name", list(gc.SCHEDULES))
def test_tangent_greeks_are_the_derivatives_of_the_frozen_price(name, is_put):
    """Central differences with relative float64 bumps of 1e-5 (absolute for r and q).  With the steps, the in-the-money
    indicator and the floor's outcome held fixed the price is smooth: a path's spot is affine in S0 and analytic in the
    others, so the truncation error delta^2 f''' / 6 is below 1e-9 relative and the rounding error 1e-16 V / delta below 1e-9
    of a Greek: 1e-6 holds with room."""
    steps = gc.SCHEDULES[name](N)
    divs = [((k - 0.5) * T / N, a, kind) for k, a, kind in steps]
    mul, cash, has = dr.schedule(T, N, divs)
    assert sorted(np.flatnonzero(has)) == sorted({k for k, _, _ in steps})
    Z = np.random.default_rng(11).standard_normal((N, PAIRS))
    h = 0.01

    def paths(S0_=S0, r=R, q=Q, sig=SIG, T_=T, alive=None):
        return gr.simulate(S0_, r, q, sig, T_, N, Z, mul, cash, has, alive)

    S = paths()
    out = gr.greeks((S, paths(S0 * (1 + h)), paths(S0 * (1 - h))), K, R, Q, T, is_put, _policy(), mul, cash, has, h,
                    sigma=SIG, Z=Z)
    tex = out["tex"][0]
    assert out["ties"] == [0, 0, 0]
    if name == "floor":  # (the live paths are left some 10 below or above the strike: every put stops early, no call does)
        dead = S[N] == 0.0
        assert 0.01 < dead.mean() < 0.99
    else:
        assert 0.05 < (tex < N).mean() < 0.95
    alive = S > 0.0
    s_k = S[tex, np.arange(S.shape[1])]
    itm = (K - s_k if is_put else s_k - K) > 0.0

    def price(r=R, T_=T, **kw):
        return gr.frozen_price(paths(r=r, T_=T_, alive=alive, **kw), K, r, T_, is_put, tex, itm)

    assert abs(price() - out["price"]) <= 1e-12 * out["price"]
    for greek, arg, x, d in (("delta", "S0_", S0, 1e-5 * S0), ("vega", "sig", SIG, 1e-5 * SIG), ("rho", "r", R, 1e-5),
                             ("epsilon", "q", Q, 1e-5), ("theta", "T_", T, 1e-5 * T)):
        fd = (price(**{arg: x + d}) - price(**{arg: x - d})) / (2.0 * d)
        want = -fd if greek == "theta" else fd
        assert abs(out[greek] - want) <= 1e-6 * abs(want), (greek, out[greek], want)
    assert math.isfinite(out["gamma"])


def test_s0_tangent_without_cash_is_the_spot_ratio_and_is_zero_behind_the_floor():
    Z = np.random.default_rng(3).standard_normal((N, 500))
    mul, cash, has = dr.schedule(T, N, [((3 - 0.5) * T / N, 0.05, "proportional")])
    S = gr.simulate(S0, R, Q, SIG, T, N, Z, mul, cash, has)
    np.testing.assert_allclose(gr.s0_tangent(S, cash, has), S / S0, rtol=1e-14)
    mul, cash, has = dr.schedule(T, N, [((2 - 0.5) * T / N, 1000.0, "cash")])
    S = gr.simulate(S0, R, Q, SIG, T, N, Z, mul, cash, has)
    Y = gr.s0_tangent(S, cash, has)
    assert np.all(S[2:] == 0.0) and np.all(Y[2:] == 0.0) and np.all(Y[:2] > 0.0)

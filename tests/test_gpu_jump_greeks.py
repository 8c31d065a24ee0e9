"""omc_price_american_jump_greeks (include/omc_jump_greeks.h) on the GPU, against the numpy
restatement (helpers/jump_greeks_ref.py) on the device's OWN matrices -- omc_price_american_jump's S_keep at S0,
S0 (1 + h) and S0 (1 - h) --, the generator's own normals and the counts and jump normals of the C oracle's Philox.

  1. the grid of helpers/jump_greeks_case.grid: pairs {1, 63, 64, 65, 257, 773}, steps {1, 2, 3, 4, 5, 8, 9, 13},
     x = lambda T / N in {1e-6, 0.05, 1}, four jump-size laws, put and call, GBM and Heston schemes 0, 1 and 3.  Counts and
     sum_nitm of omc_price_american_jump, betas_out the bits of omc_lsm_poly's fits, the price to 1e-9, price_up /
     price_down and their counts by the same rule on the bumped matrices, every Greek within TOL of the restatement.
     Jump sizes (0, 0): the counts of omc_price_american_div_greeks without dividends, its delta .. epsilon, and its theta
     against theta - theta_score.  x = 1e-6: no jump is drawn and the pathwise Greeks are those of the lambda = 0 call.
  2. lambda = 0: dmu_j = dsigma_j = theta_score = 0 exactly, dlambda NaN, the rest as omc_price_american_div_greeks
  3. the European table on the CPU test's case and seed: within 4 standard errors of Merton's series, within TOL of the
     restatement, and TOL below 1 % of every Greek's standard error there (the smallest se / |Greek| of the file)
  4. identical calls return identical bits; the call's own betas_out as betas returns the same Greeks
  5. the C error codes, *out untouched on refusal

TOL is MEASURED: the worst relative error of each Greek over 1, 3 and the fuzz sweep (DESIGN.md 34.4 lists them), times 4.
Both sides read the same float32 spots and form the terms in float64, so delta, rho, epsilon, dlambda, dmu_j and theta_score
agree to the rounding of a float64 mean (worst 4e-16).  vega and theta carry the sweep's float32 sum of the normals (1e-8).
dsigma_j carries the device's jump normal -- float32 logarithm, square root and cosine -- against the restatement's exact one
(1.1e-6).  gamma is a difference of two deltas over 2 h S0: the sweep's float32 growth product against the matrix's S_k / S_0,
1e-7 apart per delta, is amplified where both bumped chains stop in the money at different steps (1.9e-5 at one pair;
2.6e-7 and below in every other case).  Two sweeps that
each agree with their restatement within their own bound agree with each other within the sum of the two: that is the
bound of the comparisons with omc_price_american_div_greeks (DTOL is its file's)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import call_catalogue as cat
from helpers import jump_greeks_case as gc
from helpers import jump_greeks_ref as gr
from options_model_amd import _ffi
from test_gpu_dividend_greeks import TOL as DTOL

pytestmark = pytest.mark.gpu

# 4 x the worst measured relative error over the comparisons of this file and the fuzz sweep at scale 1
TOL = dict(delta=4 * 1.799e-16, gamma=4 * 1.930e-05, vega=4 * 1.227e-08, rho=4 * 2.944e-16, theta=4 * 3.228e-09,
           epsilon=4 * 3.980e-16, dlambda=4 * 1.420e-16, dmu_j=4 * 3.502e-16, dsigma_j=4 * 1.062e-06, theta_score=4 * 2.543e-16)
CAP = 0.01  # of the Greek's standard error
SUM = 1e-9  # the project's standing contract for a reordered float64 sum
H = 0.01
NAN_UNDER_HESTON = tuple(k for g in gr.GREEKS[2:] for k in (g, "se_" + g))
SHARED = ("delta", "gamma", "vega", "rho", "epsilon")  # what the dividend Greeks' sweep forms too (and theta, below)


def names_of(p, lam):
    if gc.is_heston(p):
        return ("delta", "gamma")
    return tuple(g for g in gr.GREEKS if g != "dlambda" or lam > 0.0)


def compare(ctx, p, jump, q, h, betas=None, label=""):
    """one call against the restatement on the device's own inputs -> (out, ref, mats, results of the three pricings)"""
    mats, res, Z = gc.device_inputs(ctx, p, jump, q, h)
    out = ctx.price_american_jump_greeks(p, jump, q, bump=h, betas=betas, want_betas=True)
    ref = gc.restate(p, jump, q, h, mats, Z, out["betas"])
    assert ref["ties"] == [0, 0, 0], "a decision within 1e-10 K of its continuation value: not a case for exact counts"
    for k in ("n_exercised", "n_zero", "n_exercised_up", "n_exercised_down"):
        assert out[k] == ref[k], (label, k, out[k], ref[k])
    for k in ("price", "price_up", "price_down"):
        assert abs(out[k] - ref[k]) <= SUM * abs(ref[k]), (label, k, out[k], ref[k])
    gbm = Z is not None
    if gbm:
        assert out["n_jumps"] == ref["n_jumps"], (label, out["n_jumps"], ref["n_jumps"])
    names = names_of(p, jump[0])
    err = gc.rel_errors(out, ref, names)
    print("MEASURED", label, " ".join(f"{g}={e:.3e}" for g, e in err.items()),
          " ".join(f"se/|{g}|={ref['se_' + g] / abs(ref[g]):.3e}" for g in err if ref[g] != 0.0))
    for g, e in err.items():
        assert e <= TOL[g], (label, g, out[g], ref[g], e)
        assert abs(out["se_" + g] - ref["se_" + g]) <= 1e-3 * ref["se_" + g] + 1e-300, (label, "se_" + g)
    if not gbm:
        assert math.isfinite(out["delta"]) and math.isfinite(out["gamma"])
        assert all(math.isnan(out[k]) for k in NAN_UNDER_HESTON)
    assert out["folded"] == 0 and out["ms_pass2"] == 0.0 and out["ms_greeks"] > 0.0 and out["bump"] == h
    thr, kappa, rj = _ffi.jump_table(p, jump, q)
    assert (out["kappa"], out["drift_rate"]) == (kappa, rj)
    return out, ref, mats, res


def against_dividend_greeks(ctx, p, q, h, out, betas, label, theta_of=lambda o: o["theta"]):
    """`out` against omc_price_american_div_greeks without dividends at yield q, on the same policy"""
    div = ctx.price_american_dividend_greeks(p, q, [], bump=h, betas=betas)
    for k in ("n_exercised", "n_zero", "n_exercised_up", "n_exercised_down"):
        assert out[k] == div[k], (label, k, out[k], div[k])
    for k in ("price", "price_up", "price_down"):
        assert abs(out[k] - div[k]) <= SUM * abs(div[k]), (label, k, out[k], div[k])
    gbm = not gc.is_heston(p)
    for g in SHARED if gbm else ("delta", "gamma"):
        assert abs(out[g] - div[g]) <= (TOL[g] + DTOL[g]) * abs(div[g]), (label, g, out[g], div[g])
    if gbm:
        tol = TOL["theta"] * abs(out["theta"]) + TOL["theta_score"] * abs(out["theta_score"]) + DTOL["theta"] * abs(div["theta"])
        assert abs(theta_of(out) - div["theta"]) <= tol, (label, "theta", theta_of(out), div["theta"], tol)
    return div


CASES = gc.grid()


# ------------------------------------------------------------------ 1. the grid
@pytest.mark.parametrize("c", CASES, ids=[gc.case_id(c) for c in CASES])
def test_pricing_and_greeks_against_the_restatement(ctx, c):
    N = c["N"]
    p = gc.case_params(c)
    jump = gc.jump_of(c)
    out, ref, mats, res = compare(ctx, p, jump, gc.Q, H, label=gc.case_id(c))
    base = res[0]
    assert base["folded"] == 0
    assert (out["n_exercised"], out["n_zero"], out["sum_nitm"]) == (base["n_exercised"], base["n_zero"], base["sum_nitm"])
    assert abs(out["price"] - base["price"]) <= SUM * abs(base["price"]), (out["price"], base["price"], ref["price"])
    if N >= 2:
        Sd = ctx.to_device(mats[0])
        try:
            fit = ctx.lsm_poly(Sd, p.K, p.r, p.T, bool(p.is_put), "two_pass")
        finally:
            Sd.free()
        np.testing.assert_array_equal(out["betas"][:, :3].view(np.uint64), np.ascontiguousarray(fit["betas"]).view(np.uint64))
        np.testing.assert_array_equal(out["betas"][:, 3].astype(np.int64), fit["nitm"])
    lam, mu, sj = jump
    kappa = out["kappa"]
    if c["x"] == 1e-6:
        # no count word passes thr[0] = 2^24 - 17 or so: the paths are the vanilla ones at the drift rate (r - q) - lambda kappa,
        # which the lambda = 0 call takes at the yield q + lambda kappa.  Its theta has no score part.
        assert out["n_jumps"] == 0
        zero = ctx.price_american_jump_greeks(p, (0.0, mu, sj), gc.Q + lam * kappa, bump=H, betas=out["betas"])
        for k in ("n_exercised", "n_zero", "n_exercised_up", "n_exercised_down"):
            assert out[k] == zero[k], k
        for g in (SHARED if not gc.is_heston(p) else ("delta", "gamma")):
            assert abs(out[g] - zero[g]) <= TOL[g] * abs(zero[g]), (g, out[g], zero[g])
        if not gc.is_heston(p):
            tol = TOL["theta"] * abs(zero["theta"]) + TOL["theta_score"] * abs(out["theta_score"])
            assert abs(out["theta"] - out["theta_score"] - zero["theta"]) <= tol
    if (mu, sj) == (0.0, 0.0):
        against_dividend_greeks(ctx, p, gc.Q, H, out, out["betas"], gc.case_id(c), lambda o: o["theta"] - o["theta_score"])


# ------------------------------------------------------------------ 2. lambda = 0
@pytest.mark.parametrize("model,is_put,N,pairs", [("gbm", True, 5, 773), ("gbm", False, 13, 257), ("heston0", True, 4, 65),
                                                  ("heston3", False, 9, 773)])
def test_without_intensity_the_jump_greeks_vanish(ctx, model, is_put, N, pairs):
    p = gc.make_params(model, is_put=is_put, N=N, M=2 * pairs, seed=77, sigma=0.25)
    out = ctx.price_american_jump_greeks(p, (0.0, -0.1, 0.15), gc.Q, bump=H, want_betas=True)
    assert out["n_jumps"] == 0 and out["folded"] == 0 and out["drift_rate"] == p.r - gc.Q
    if model == "gbm":
        assert out["dmu_j"] == 0.0 and out["dsigma_j"] == 0.0 and out["theta_score"] == 0.0
        assert out["se_dmu_j"] == 0.0 and out["se_dsigma_j"] == 0.0 and out["se_theta_score"] == 0.0
        assert math.isnan(out["dlambda"]) and math.isnan(out["se_dlambda"])
        assert all(math.isfinite(out[g]) for g in SHARED + ("theta",))
    else:
        assert all(math.isnan(out[k]) for k in NAN_UNDER_HESTON)
    div = against_dividend_greeks(ctx, p, gc.Q, H, out, out["betas"], f"lambda0-{model}")
    fit = ctx.price_american_dividend_greeks(p, gc.Q, [], bump=H, want_betas=True)  # and the fits are its own
    np.testing.assert_array_equal(out["betas"].view(np.uint64), fit["betas"].view(np.uint64))
    assert out["sum_nitm"] == fit["sum_nitm"] and div["sum_nitm"] == 0


# ------------------------------------------------------------------ 3. the European table: Merton's series
@pytest.mark.parametrize("is_put", [True, False], ids=["put", "call"])
def test_european_table_is_mertons_series(ctx, is_put):
    e = gc.EURO
    p = gc.euro_params(is_put)
    jump = (e["lam"], e["mu_j"], e["sigma_j"])
    out, ref, _, _ = compare(ctx, p, jump, e["q"], e["h"], betas=gc.european(e["N"]), label=f"european-{is_put}")
    assert out["n_exercised"] == 0 and out["sum_nitm"] == 0 and out["n_jumps"] > 0
    want = gc.euro_closed_form(is_put)
    se = dict(ref, se_price=ref["se_price"])
    for k in gc.EURO_NAMES:
        print("EUROPEAN", k, out[k], ref[k], want[k], se["se_" + k])
        assert abs(out[k] - want[k]) <= 4.0 * se["se_" + k], (k, out[k], want[k], se["se_" + k])
    # the largest sample of the file: se / |Greek| is smallest here.  A tolerance near the Monte-Carlo error would hide a
    # wrong term
    for g in gr.GREEKS:
        print("CAP", g, TOL[g] * abs(ref[g]) / ref["se_" + g])
        assert TOL[g] * abs(ref[g]) <= CAP * ref["se_" + g], (g, "the tolerance is not below 1 % of the standard error")


# ------------------------------------------------------------------ 4. identical bits
@pytest.mark.parametrize("model", ["gbm", "heston3"])
def test_identical_calls_return_identical_bits(ctx, model):
    p = gc.make_params(model, N=13, M=2 * 773, seed=31, sigma=0.25)
    jump = (6.0, -0.1, 0.15)
    a = ctx.price_american_jump_greeks(p, jump, 0.02, bump=H, want_betas=True)
    b = ctx.price_american_jump_greeks(p, jump, 0.02, bump=H, want_betas=True)
    assert cat.diff(cat.flat(a), cat.flat(b)) == []
    g = ctx.price_american_jump_greeks(p, jump, 0.02, bump=H, betas=a["betas"], want_betas=True)
    assert g["sum_nitm"] == 0 and a["sum_nitm"] > 0 and a["n_jumps"] > 0
    fa, fg = cat.flat(a), cat.flat(g)
    for d in (fa, fg):
        d.pop("sum_nitm")
    assert cat.diff(fa, fg) == []


# ------------------------------------------------------------------ 5. the C error codes
def test_error_codes_leave_the_result_untouched(ctx):
    lib = ctx.lib
    p = gc.make_params("gbm", N=7, M=2048, seed=1)
    out = _ffi.JumpGreeks()
    size = C.sizeof(out)

    def call(pp=p, jump=(1.0, -0.1, 0.15), q=0.0, bump=0.01, res=out, handle=None, j_null=False):
        C.memset(C.byref(out), 0xA5, size)
        rc = lib.omc_price_american_jump_greeks(handle or ctx.handle, C.byref(pp), None if j_null else C.byref(_ffi.make_jump(jump)),
                                                float(q), float(bump), None, None, C.byref(res) if res is not None else None)
        if rc != 0:
            assert bytes(out) == b"\xA5" * size, rc  # nothing was written
        return rc

    assert call() == 0 and out.g.base.price > 0.0 and out.n_jumps > 0
    assert [call(bump=b) for b in (0.0, 0.6, math.nan, -0.01)] == [-4] * 4
    assert call(bump=0.5) == 0
    assert call(res=None) == -7
    assert call(j_null=True) == -25 and call(q=math.nan) == -17
    assert call(jump=(-1.0, 0.0, 0.1)) == -26 and call(jump=(math.inf, 0.0, 0.1)) == -26
    assert call(jump=(1.0, math.nan, 0.1)) == -27 and call(jump=(1.0, 0.0, -0.1)) == -27
    assert call(jump=(7.5, 0.0, 0.1)) == -28 and call(jump=(7.0, 0.0, 0.1)) == 0
    assert call(pp=gc.with_(p, antithetic=0)) == -24
    assert call(pp=gc.with_(p, semantics=_ffi.SEMANTICS["reference"])) == -11
    assert call(pp=gc.with_(p, n_paths=2047)) == -3
    # the law's refusals come before the bump's
    assert call(q=math.nan, bump=0.0) == -17
    c = _ffi.Context(0)
    try:
        c.set_allreduce_hook(lambda dptr, count: None)
        assert call(handle=c.handle) == -10
        c.set_allreduce_hook(None)
        assert call(handle=c.handle) == 0
    finally:
        c.close()
    with pytest.raises(ValueError):
        ctx.price_american_jump_greeks(p, (1.0, 0.0, 0.1), 0.0, betas=np.zeros((5, 4)))
    assert call() == 0  # and the context still prices


def test_facade_returns_the_ffi_numbers(ctx):
    from options_model_amd import JumpGreeksResult, price_american_jump_greeks
    for model in ("GBM", "Heston"):
        r = price_american_jump_greeks(100.0, 100.0, 0.05, 0.2, 1.0, 4096, 12, 2.0, jump_mean=-0.1, jump_vol=0.15,
                                       dividend_yield=0.01, model=model, option_type="put", seed=5, bump=0.02, ctx=ctx)
        p = _ffi.make_params(model=model.lower(), is_put=True, semantics="two_pass", n_paths=4096, n_steps=12, S0=100.0, K=100.0,
                             r=0.05, sigma=0.2, T=1.0, seed=5, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
        o = ctx.price_american_jump_greeks(p, (2.0, -0.1, 0.15), 0.01, bump=0.02, want_betas=True)
        assert isinstance(r, JumpGreeksResult) and float(r) == r.price == o["price"]
        for k in ("delta", "gamma", "se_delta", "se_gamma", "price_up", "price_down", "n_exercised_up", "n_exercised_down", "bump",
                  "n_jumps", "kappa", "drift_rate"):
            assert getattr(r, k) == o[k], k
        for k in gr.GREEKS[2:]:
            assert getattr(r, k) == o[k] or (math.isnan(getattr(r, k)) and math.isnan(o[k])), k
        assert r.n_paths == 4096 and r.jump_intensity == 2.0
        np.testing.assert_array_equal(r.betas, o["betas"])

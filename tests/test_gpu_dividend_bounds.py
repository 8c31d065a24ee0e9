"""Andersen-Broadie price bounds for a stock that pays discrete dividends (omc_price_american_bounds_div,
omc_dividend_paths_f32; options_model_amd/csrc/omc_dividend_bounds.hip).

The generator against omc_price_american_div's kept matrix (bits), with and without the variance state, against the vanilla
generators where no dividend is paid, and started at a later date against the same call on the schedule shifted in time; the
device's Q^_t, samples, bounds and counts against the numpy restatements of tests/helpers/bounds_ref.py,
bounds_schedule_ref.py and bounds_check_ref.py on the device's own spots (tests/helpers/dividend_bounds_case.py;
tests/test_gpu_dividend_bounds_fuzz.py runs the same comparison over random shapes); the degenerate laws against the
dividend-free bounds, bit for bit; known answers; the refusals; determinism; the facade.  Every case at a small shape."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_check_ref as bk
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs
from helpers import dividend_bounds_case as dc
from helpers import dividend_known as dk
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
Q = 0.03
OUT_KEYS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
            "inner_path_steps")
GEN_MODELS = ("gbm", "heston0", "heston1", "heston2", "heston3")  # the generator takes every scheme


def _params(model="gbm", is_put=True, S0=100.0, N=8, M=2000, seed=42, stream=0, hp=None):
    hp = hp or (dc.HP_CLAMP if model == "heston1" else dc.HP)  # scheme 1 with the Feller-violating set
    return dc.make_params(model, is_put=is_put, S0=S0, K=K, r=R, sigma=SIG, T=T, N=N, M=M, seed=seed, stream=stream, hp=hp)


def _divs(N, steps=None):
    """a mixed schedule on N steps: by default a cash dividend on step 1, cash + proportional on the middle step, cash on N"""
    if steps is None:
        mid = (N + 1) // 2
        steps = [(1, 1.5, "cash"), (mid, 1.0, "cash"), (mid, 0.02, "proportional"), (N, 2.0, "cash")]
    return dc.dividends_at(steps, T, N)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, keys=OUT_KEYS, arrays=("betas", "q", "samples")):
    for key in keys:
        assert a[key] == b[key], key
    for key in arrays:
        if key in a or key in b:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _vanilla(ctx, p, q):
    """the vanilla generator's matrix of p at rate r - q (and the variance state under Heston schemes 0 .. 2)"""
    M, N = int(p.n_paths), int(p.n_steps)
    if not dc.is_heston(p):
        return dc.host(ctx.gbm_paths(M, N, p.S0, p.r - q, p.sigma, p.T, p.seed, p.stream, p.pair_offset)), None
    h = dc.hc.hp_of(p)
    S = dc.host(ctx.heston_paths(M, N, p.S0, p.r - q, p.T, *h, p.seed, p.stream, p.pair_offset, int(p.heston_scheme)))
    Sv, Vv = ctx.heston_paths_sv(M, N, p.S0, p.r - q, p.T, *h, p.seed, p.stream, p.pair_offset, int(p.heston_scheme))
    Sv.free()
    return S, dc.host(Vv)


# ---------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize("model", GEN_MODELS)
@pytest.mark.parametrize("M,N", [(4096, 13), (1000, 9), (12, 4), (10, 3), (2, 1)])  # (stores 4, 4, 2, 1, 1 pairs wide)
def test_generator_is_the_pricing_calls_matrix_with_and_without_the_variance(ctx, model, M, N):
    p = dc.with_(_params(model, N=N, M=M, seed=9, stream=5), pair_offset=3)
    divs = _divs(N)
    keep = ctx.empty((N + 1, M), np.float32)
    ctx.price_american_div(p, Q, divs, S_keep=keep)
    ref = dc.host(keep)
    S = dc.host(ctx.dividend_paths(p, Q, divs))
    np.testing.assert_array_equal(_bits(S), _bits(ref))
    assert np.any(S != dc.host(ctx.dividend_paths(p, Q, ())))  # (the dividends are there)
    if dc.is_heston(p):
        Sd, Vd = ctx.dividend_paths(p, Q, divs, want_v=True)
        S2, V = dc.host(Sd), dc.host(Vd)
        np.testing.assert_array_equal(_bits(S2), _bits(ref))
        assert V.shape == S.shape and np.all(V[0] == np.float32(p.v0)) and np.all(np.isfinite(V))
        # a dividend leaves the variance alone: the state is the dividend-free generator's at the same drift rate
        np.testing.assert_array_equal(_bits(V), _bits(_vanilla(ctx, p, Q)[1]))


@pytest.mark.parametrize("model", ["gbm", "heston1", "heston3"])
def test_generator_with_an_odd_leading_dimension(ctx, model):
    M, N, ld = 10, 5, 13
    p = _params(model, N=N, M=M, seed=9)
    arr, n = _ffi.dividend_array(_divs(N))
    ref = dc.host(ctx.dividend_paths(p, Q, _divs(N)))
    S = ctx.to_device(np.full((N + 1, ld), np.float32(-7.0)))
    V = ctx.to_device(np.full((N + 1, ld), np.float32(-7.0)))
    v = V.ptr if dc.is_heston(p) else None
    assert ctx.lib.omc_dividend_paths_f32(ctx.handle, C.byref(p), Q, arr, n, 0, S.ptr, v, ld) == 0
    got, gv = dc.host(S), dc.host(V)
    np.testing.assert_array_equal(_bits(got[:, :M]), _bits(ref))
    assert np.all(got[:, M:] == -7.0) and np.all(gv[:, M:] == -7.0)  # (the padding is not written)


@pytest.mark.parametrize("model", GEN_MODELS)
def test_no_dividend_writes_the_vanilla_matrix(ctx, model):
    """n_div = 0 and all-zero amounts: the vanilla generators at rate r - q, bit for bit"""
    M, N = 1000, 9
    p = dc.with_(_params(model, N=N, M=M, seed=11, stream=2), pair_offset=17)
    ref, vref = _vanilla(ctx, p, Q)
    zero = dc.dividends_at([(1, 0.0, "cash"), (4, 0.0, "proportional"), (5, 0.0, "cash"), (9, 0.0, "cash")], T, N)
    for divs in ((), zero):
        np.testing.assert_array_equal(_bits(dc.host(ctx.dividend_paths(p, Q, divs))), _bits(ref))
        if dc.is_heston(p):
            Sd, Vd = ctx.dividend_paths(p, Q, divs, want_v=True)
            np.testing.assert_array_equal(_bits(dc.host(Sd)), _bits(ref))
            np.testing.assert_array_equal(_bits(dc.host(Vd)), _bits(vref))


@pytest.mark.parametrize("model", dc.MODELS)
def test_a_start_date_shifts_the_schedule(ctx, model):
    """step_offset = t: row k takes the entry of step t + k, and the entry of step t itself is not applied -- the same call at
    step_offset = 0 on the schedule moved t steps back in time, without the dividends that have gone ex by then, bit for bit.
    The vanilla step does not depend on the date, so with the pricing call's matrix at offset 0 this is the restart property:
    a path that starts at date t in the state of row t continues as rows t .. N do."""
    M, N = 1000, 13
    steps = [(1, 1.5, "cash"), (4, 1.0, "cash"), (5, 0.02, "proportional"), (5, 0.7, "cash"), (8, 30.0, "cash"), (13, 2.0, "cash")]
    p = dc.with_(_params(model, N=N, M=M, seed=3, stream=4), pair_offset=5)
    for t in range(N + 1):
        later = [(k - t, a, kind) for k, a, kind in steps if k > t]
        want_v = dc.is_heston(p)
        a = ctx.dividend_paths(p, Q, dc.dividends_at(steps, T, N), step_offset=t, want_v=want_v)
        b = ctx.dividend_paths(p, Q, dc.dividends_at(later, T, N), want_v=want_v)
        for x, y in zip(a if want_v else (a,), b if want_v else (b,)):
            np.testing.assert_array_equal(_bits(dc.host(x)), _bits(dc.host(y)), err_msg=f"t {t}")


@pytest.mark.parametrize("model", ["heston0", "heston1"])
def test_a_stored_state_is_a_start_state(ctx, model):
    """(S[t, j], V[t, j]) -- under scheme 1 with the Feller-violating set some of them negative -- come back as row 0 of both
    partners, not validated, not floored, and no dividend is applied to them"""
    M, N, off = 1000, 13, 7
    P = M // 2
    divs = _divs(N)
    p = dc.with_(_params(model, N=N, M=M, stream=5), pair_offset=off)
    Sd, Vd = ctx.dividend_paths(p, Q, divs, want_v=True)
    S, V = dc.host(Sd), dc.host(Vd)
    assert (V.min() < 0.0) == (model == "heston1")
    for t in (0, 1, 7, 13):  # (1, 7 and 13 are dividend steps of the schedule)
        low = np.argsort(np.minimum(V[t, :P], V[t, P:]))[:3]
        for j in sorted({0, P - 1, *[int(x) for x in low]}):
            for col in (j, j + P):
                g = dc.with_(p, n_paths=2, S0=float(S[t, col]), v0=float(V[t, col]), pair_offset=off + j)
                Xd, Wd = ctx.dividend_paths(g, Q, divs, step_offset=t, want_v=True)
                X, W = dc.host(Xd), dc.host(Wd)
                assert np.all(_bits(X[0]) == _bits(S[t, col:col + 1])) and np.all(_bits(W[0]) == _bits(V[t, col:col + 1]))
                assert X.shape == (N + 1, 2) and np.all(np.isfinite(X)) and np.all(X >= 0)


def test_generator_refusals(ctx):
    lib, hnd = ctx.lib, ctx.handle
    S, V = ctx.empty((4, 10), np.float32), ctx.empty((4, 10), np.float32)
    g, h = _params("gbm", N=3, M=10), _params("heston1", N=3, M=10)
    arr, n = _ffi.dividend_array(_divs(3))

    def call(p, q=Q, d=arr, nd=n, off=0, s=S.ptr, v=None, ld=10):
        return lib.omc_dividend_paths_f32(hnd, C.byref(p), float(q), d, nd, off, s, v, ld)

    def one(t, amount, kind):
        return _ffi.dividend_array([(t, amount, kind)])[0]

    try:
        assert call(g) == 0 and call(h) == 0 and call(h, v=V.ptr) == 0 and call(g, d=None, nd=0) == 0
        assert call(g, off=3) == 0 and call(g, off=-1) == -41 and call(g, off=4) == -41
        assert b"step_offset" in lib.omc_last_error()
        assert call(g, v=V.ptr) == -7  # a variance matrix under GBM
        assert call(dc.with_(g, S0=0.0)) == 0 and call(dc.with_(g, S0=-1.0)) == -1  # a spot of 0 is a start state
        assert call(g, s=None) == -7 and call(g, ld=9) == -6
        assert call(g, q=float("nan")) == -17 and call(g, nd=-1) == -18 and call(g, d=None) == -19
        assert call(g, d=one(0.0, 1.0, "cash"), nd=1) == -20 and call(g, d=one(1.5, 1.0, "cash"), nd=1) == -20
        assert call(g, d=one(0.5, -1.0, "cash"), nd=1) == -21 and call(g, d=one(0.5, 1.0, "proportional"), nd=1) == -22
        assert call(g, d=one(0.5, 1.0, 7), nd=1) == -23
        assert call(dc.with_(g, n_paths=9)) == -3 and call(dc.with_(g, antithetic=0)) == -24
        assert call(g, off=-1, q=float("nan")) == -17  # the dividend argument errors come first
        for sem in (0, 1, 2):
            assert call(dc.with_(g, semantics=sem)) == 0  # the semantics are not used
        assert call(dc.with_(g, semantics=3)) == -4
        # v0 is a start state under schemes 0 .. 2; QE keeps its check
        for scheme in (0, 1, 2):
            assert call(dc.with_(h, heston_scheme=scheme, v0=-0.01), v=V.ptr) == 0
        qe = dc.with_(h, heston_scheme=3, xi=1.0)
        assert call(qe, v=V.ptr) == 0 and call(dc.with_(qe, v0=-0.01)) == -5
        assert call(dc.with_(h, heston_scheme=4)) == -4
    finally:
        S.free()
        V.free()


# ---------------------------------------------------------------------------------------------- 2. the restatement
def _run_case(ctx, c, **kw):
    p, divs = dc.case_params(c), dc.dividends_of(c)
    given = dc.given_table(ctx, p, c["q"], divs, c["holes"]) if c["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", c["irr_every"])
    try:
        d = ctx.price_american_bounds_div(p, c["q"], divs, policy=c["policy"], n_lower=c["n_lower"], n_outer=c["n_outer"],
                                          n_inner=c["n_inner"], betas=given, want_q=True, want_samples=True, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    return p, divs, given, d


@pytest.mark.parametrize("c", dc.DIRECTED, ids=[dc.case_id(c) for c in dc.DIRECTED])
def test_device_equals_restatement(ctx, c):
    p, divs, given, d = _run_case(ctx, c)
    if given is not None:
        np.testing.assert_array_equal(d["betas"], given)
    else:  # omc_lsm_poly's fits on the dividend paths of p
        np.testing.assert_array_equal(d["betas"], dc.fitted_table(ctx, p, c["q"], divs, c["policy"]))
    sp = dc.device_spots(ctx, p, c["q"], divs, c["n_lower"], c["n_outer"], c["n_inner"])
    dc.check_against_restatement(p, d, sp, c["n_lower"], c["n_outer"], c["n_inner"])
    zeros = float(np.mean(sp["Sl"][-1] == 0.0))
    if c in dc.ABSORBING:  # the large dividend takes spots to exactly 0, where they stay; items start there too
        assert 0.01 < zeros < 0.5 and np.any(sp["So"][:-1] == 0.0)
        k0 = min(dc.steps_of(c))
        assert np.all(sp["Sl"][k0:][:, sp["Sl"][k0] == 0.0] == 0.0)
    print(f"{dc.case_id(c)}: bounds [{d['lower']:.4f}, {d['upper']:.4f}], inner steps {d['inner_path_steps']}, "
          f"lower paths at 0: {zeros:.3f}")


# ---------------------------------------------------------------------------------------------- 3. an exercise schedule
@pytest.mark.parametrize("model", dc.MODELS)
@pytest.mark.parametrize("k", [2, 3, 9, 14])
def test_schedule_equals_restatement_and_the_masked_call(ctx, model, k):
    N, n_lower, n_outer, n_inner = 9, 1000, 6, 130
    is_put = k != 3
    p = _params(model, is_put=is_put, N=N, S0=100.0 if is_put else 104.0)
    divs = _divs(N, [(2, 1.5, "cash"), (3, 0.02, "proportional"), (6, 2.0, "cash"), (9, 1.0, "cash")])
    policy = {2: "textbook", 3: "two_pass", 9: "reference", 14: "textbook"}[k]
    kw = dict(n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True)
    d = ctx.price_american_bounds_div(p, Q, divs, policy=policy, exercise_every=k, **kw)
    assert ctx._bounds_every == 0
    np.testing.assert_array_equal(d["betas"], dc.fitted_table(ctx, p, Q, divs, policy, k))
    taus = bs.schedule(N, k)
    sp = dc.device_spots(ctx, p, Q, divs, n_lower, n_outer, n_inner, ts=taus[:-1])
    bs.check_against_restatement(p, d, sp, k, n_lower, n_outer, n_inner)
    # the all-dates call given the scheduled table (zero rows off the schedule): the same stops, the same Q^ where both have one
    A = ctx.price_american_bounds_div(p, Q, divs, policy="given", betas=d["betas"], **kw)
    for key in ("lower", "se_lower", "n_exercised_lower"):
        assert d[key] == A[key], key
    on = taus[:-1]
    np.testing.assert_array_equal(d["q"][:, on], A["q"][:, on])
    assert np.all(d["q"][:, [t for t in range(N) if t not in on]] == 0.0)
    assert d["inner_path_steps"] <= A["inner_path_steps"]


# ---------------------------------------------------------------------------------------------- 4. the payoff check
@pytest.mark.parametrize("model,N,n_inner,is_put,S0", [("gbm", 9, 130, True, 100.0), ("gbm", 4, 64, False, 110.0),
                                                       ("heston0", 13, 64, True, 90.0), ("heston1", 5, 200, False, 100.0),
                                                       ("heston1", 1, 2, True, 100.0)])
def test_payoff_check_against_the_dense_call(ctx, model, N, n_inner, is_put, S0):
    n_lower, n_outer = 1000, 6
    p = _params(model, is_put=is_put, N=N, S0=S0)
    divs = _divs(N)
    kw = dict(policy="textbook", n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True)
    dense = ctx.price_american_bounds_div(p, Q, divs, **kw)
    got = ctx.price_american_bounds_div(p, Q, divs, suboptimality_check="payoff", **kw)
    assert ctx._bounds_check == 0
    sp = dc.device_spots(ctx, p, Q, divs, n_lower, n_outer, n_inner)
    dc.check_against_restatement(p, dense, sp, n_lower, n_outer, n_inner)
    st = bk.item_steps(sp["So"], sp["inner"], range(n_outer), K, R, T, is_put, dense["betas"])
    assert st["ties"] == 0
    kp = bk.check_against_dense(p, dense, got, 1, sp["So"], None, st["steps"])  # (lower and every kept mean keep their bits)
    up = bk.upper_bound(sp["So"], sp["inner"], 1, K, R, T, is_put, got["betas"])
    assert up["ties"] == 0 and got["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(got["q"], up["q"], rtol=1e-12, atol=1e-12 * K)
    # upper_checked <= upper up to the walk's rounding (tests/test_gpu_bounds_check.py's tolerance)
    assert np.all(got["samples"] <= dense["samples"] + br.samples_atol(N, dense["q"], K) + bk.WALK_RTOL * K)
    assert got["upper"] <= dense["upper"] + br.samples_atol(N, dense["q"], K) + bk.WALK_RTOL * K
    print(f"{model} N={N}: items kept {kp.mean():.3f}, upper {got['upper']:.6f} (dense {dense['upper']:.6f})")


# ---------------------------------------------------------------------------------------------- 5. the degenerate laws
FORMS = (dict(policy="textbook"), dict(policy="two_pass", exercise_every=3), dict(policy="reference", suboptimality_check="payoff"))


@pytest.mark.parametrize("model", dc.MODELS)
@pytest.mark.parametrize("zero", [False, True], ids=["no-dividends", "zero-amounts"])
def test_degenerate_laws_carry_the_dividend_free_bits(ctx, model, zero):
    """q = 0 with n_div = 0, and with amounts of 0 on steps 1, 4, 5 and N -- the dividend branch runs and changes no bit: every
    output of the dividend-free bounds call, the schedule and the payoff check included"""
    N = 9
    p = _params(model, N=N)
    divs = dc.dividends_at([(1, 0.0, "cash"), (4, 0.0, "proportional"), (5, 0.0, "cash"), (9, 0.0, "cash")], T, N) if zero else ()
    for kw in FORMS:
        kw = dict(kw, n_lower=1000, n_outer=40, n_inner=130, want_q=True, want_samples=True)
        a = ctx.price_american_bounds_div(p, 0.0, divs, **kw)
        _same_bits(a, bs.price(ctx, p, **kw))
        assert a["inner_path_steps"] > 0
    c = dc.with_(p, is_put=0)
    given = dc.given_table(ctx, c, 0.0, divs, [t % 3 == 1 for t in range(N + 1)])
    kw = dict(policy="given", betas=given, n_lower=1000, n_outer=6, n_inner=200, want_q=True, want_samples=True)
    _same_bits(ctx.price_american_bounds_div(c, 0.0, divs, **kw), bs.price(ctx, c, **kw))


@pytest.mark.parametrize("model", dc.MODELS)
def test_yield_only_equals_the_jump_bounds_without_jumps(ctx, model):
    """n_div = 0 at q = 0.03 against omc_price_american_bounds_jump at lambda = 0 and the same q: both are the vanilla step at
    rate r - q, bit for bit"""
    p = _params(model, N=9)
    for kw in FORMS:
        kw = dict(kw, n_lower=1000, n_outer=40, n_inner=130, want_q=True, want_samples=True)
        _same_bits(ctx.price_american_bounds_div(p, Q, (), **kw), ctx.price_american_bounds_jump(p, (0.0, 0.0, 0.0), Q, **kw))


# ---------------------------------------------------------------------------------------------- 6. known answers
STAT = dict(n_lower=200_000, n_outer=2048, n_inner=256)


@pytest.mark.parametrize("is_put", [True, False])
def test_never_exercising_policy_gives_the_european_value(ctx, is_put):
    """a table of n = 0 rows never stops before N: lower is the European Monte-Carlo value, which with proportional dividends and
    a yield is Black-Scholes at S0 prod(1 - delta_i) and q"""
    N = 8
    p = _params("gbm", is_put=is_put, N=N, seed=1234)
    divs = dc.dividends_at([(2, 0.02, "proportional"), (5, 0.03, "proportional"), (8, 0.01, "proportional")], T, N)
    d = ctx.price_american_bounds_div(p, Q, divs, policy="given", betas=np.zeros((N + 1, 4)), n_lower=200_000, n_outer=2,
                                      n_inner=2)
    ref = dk.european_proportional(100.0, K, R, Q, SIG, T, [0.02, 0.03, 0.01], is_put)
    print(f"put={is_put}: lower {d['lower']:.5f} +- {d['se_lower']:.5f}, closed form {ref:.5f}")
    assert d["n_exercised_lower"] == 0
    assert abs(d["lower"] - ref) <= 4 * d["se_lower"], (d["lower"], d["se_lower"], ref)


def test_bracket_contains_the_call_with_one_proportional_dividend(ctx):
    """known answer (b) of tests/helpers/dividend_known.py: the interval contains it, the fitted textbook policy's lower bound is
    at or below it within 4 standard errors, and upper >= lower - 3 se"""
    N, k, delta, S0 = 8, 5, 0.06, 100.0
    ref = dk.bermudan_call_one_proportional(S0, K, R, SIG, T, N, k, delta)
    p = _params("gbm", is_put=False, N=N, M=100_000, S0=S0, seed=77)
    d = ctx.price_american_bounds_div(p, 0.0, dc.dividends_at([(k, delta, "proportional")], T, N), policy="textbook", **STAT)
    print(f"value {ref:.5f}: lower {d['lower']:.5f} +- {d['se_lower']:.5f}, upper {d['upper']:.5f} +- {d['se_upper']:.5f}")
    assert d["ci_lo"] <= ref <= d["ci_hi"], (d["ci_lo"], ref, d["ci_hi"])
    assert d["lower"] <= ref + 4 * d["se_lower"]
    assert d["upper"] >= d["lower"] - 3 * math.hypot(d["se_lower"], d["se_upper"])


@pytest.mark.parametrize("is_put", [True, False])
def test_bracket_contains_the_value_with_one_cash_dividend(ctx, is_put):
    """known answer (c) of tests/helpers/dividend_known.py, a float64 backward induction at N = 6 with a cash dividend of 4 on
    step 3: the interval contains it, up to the induction's own grid-doubling difference"""
    N, k, amount = 6, 3, 4.0
    a, ref = (dk.bermudan_one_dividend_grid(100.0, K, R, SIG, T, N, k, amount, "cash", is_put, m=m, nz=nz)
              for m, nz in ((1500, 1201), (3000, 2401)))
    margin = abs(ref - a)
    p = _params("gbm", is_put=is_put, N=N, M=100_000, seed=78)
    d = ctx.price_american_bounds_div(p, 0.0, dc.dividends_at([(k, amount, "cash")], T, N), policy="textbook", **STAT)
    print(f"put={is_put}: value {ref:.5f} (+- {margin:.5f}): lower {d['lower']:.5f} +- {d['se_lower']:.5f}, "
          f"upper {d['upper']:.5f} +- {d['se_upper']:.5f}")
    assert d["ci_lo"] - margin <= ref <= d["ci_hi"] + margin, (d["ci_lo"], ref, d["ci_hi"])


# ---------------------------------------------------------------------------------------------- 7. refusals
SENTINEL = 0xAB


def _raw(ctx, p, divs=None, q=Q, policy=1, regressors=0, n_lower=1000, n_outer=6, n_inner=64, betas=None, null=(), n_div=None):
    """the C call with sentinel-filled outputs -> (rc, outputs untouched?)"""
    N = int(p.n_steps)
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    C.memset(C.byref(out), SENTINEL, C.sizeof(out))
    bo, qo, so = (np.full(shape, np.nan) for shape in ((N + 1, 4), (max(n_outer, 1), N), (max(n_outer, 1),)))
    arr, n = _ffi.dividend_array(_divs(N) if divs is None else divs)
    if "divs" in null:
        arr = None
    b = None if betas is None else np.ascontiguousarray(betas, np.float64)
    rc = ctx.lib.omc_price_american_bounds_div(ctx.handle, C.byref(p), float(q), arr, n if n_div is None else n_div,
                                               None if "cfg" in null else C.byref(cfg),
                                               b.ctypes.data if b is not None else None, bo.ctypes.data, qo.ctypes.data,
                                               so.ctypes.data, None if "out" in null else C.byref(out))
    untouched = bytes(out) == bytes([SENTINEL]) * C.sizeof(out) and all(np.isnan(a).all() for a in (bo, qo, so))
    return rc, untouched


def test_refusals_leave_the_outputs_alone(ctx):
    p = _params("gbm")
    h = _params("heston0")
    nan = float("nan")
    cases = [(dict(null=("cfg",)), -7), (dict(null=("out",)), -7), (dict(q=nan), -17), (dict(n_div=-1), -18),
             (dict(null=("divs",)), -19), (dict(divs=[(0.0, 1.0)]), -20), (dict(divs=[(1.5, 1.0)]), -20),
             (dict(divs=[(0.5, -1.0)]), -21), (dict(divs=[(0.5, nan)]), -21), (dict(divs=[(0.5, 1.0, "proportional")]), -22),
             (dict(divs=[(0.5, 1.0, 7)]), -23), (dict(regressors=1), -4), (dict(policy=7), -4), (dict(policy=3), -7),
             (dict(n_inner=63), -3), (dict(n_outer=7), -3), (dict(n_lower=999), -3),
             # the dividend argument errors come before the bounds' own
             (dict(q=nan, policy=7), -17), (dict(divs=[(1.5, 1.0)], n_inner=63), -20), (dict(divs=[(0.5, -1.0)], policy=3), -21),
             (dict(n_div=-1, regressors=1), -18)]
    for kw, code in cases:
        for pp in (p, h):
            rc, untouched = _raw(ctx, pp, **kw)
            assert rc == code and untouched, (kw, rc)
    assert _raw(ctx, dc.with_(p, antithetic=0))[0] == -24
    assert _raw(ctx, dc.with_(p, sigma=0.0))[0] == -5
    for scheme in (2, 3):
        rc, untouched = _raw(ctx, dc.with_(h, heston_scheme=scheme))
        assert rc == -12 and untouched
    assert _raw(ctx, _params("gbm", N=252), n_outer=1 << 14, n_inner=1 << 12) == (-16, True)
    assert _raw(ctx, _params("gbm", N=252), n_outer=1 << 14, n_inner=1 << 12, q=nan) == (-17, True)
    assert _raw(ctx, dc.with_(p, semantics=0))[0] == 0  # p->semantics is not used
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _raw(hooked, p) == (-10, True)
        assert _raw(hooked, p, q=nan) == (-17, True)
    finally:
        hooked.close()


def test_option_refusals_and_the_way_back(ctx):
    kw = dict(n_lower=1000, n_outer=6, n_inner=64, want_q=True, want_samples=True)
    pairs = [(_params(m), m) for m in dc.MODELS]
    divs = _divs(8)
    before = {m: ctx.price_american_bounds_div(p, Q, divs, **kw) for p, m in pairs}
    try:
        ctx.set_option("bounds_control_variate", 1)
        for p, m in pairs:
            assert _raw(ctx, p) == (-39, True), m
            assert b"bounds_control_variate" in ctx.lib.omc_last_error()
            assert _raw(ctx, p, n_inner=63) == (-3, True)  # the call's own checks come first
        ctx.set_option("bounds_control_variate", 0)
        ctx.set_option("bounds_suboptimality", 2)
        for p, m in pairs:
            assert _raw(ctx, p) == (-40, True), m
            assert b"bounds_suboptimality" in ctx.lib.omc_last_error()
            assert _raw(ctx, dc.with_(p, n_paths=0)) == (-3, True)
        ctx.set_option("bounds_suboptimality", 1)
        ctx.set_option("bounds_exercise_every", 2)
        for p, m in pairs:
            assert _raw(ctx, p) == (-40, True), m  # a schedule and a check exclude each other
        ctx.set_option("bounds_exercise_every", 0)
        assert _raw(ctx, pairs[0][0])[0] == 0
    finally:
        ctx.set_option("bounds_exercise_every", 0)
        ctx.set_option("bounds_control_variate", 0)
        ctx.set_option("bounds_suboptimality", 0)
    with pytest.raises(ValueError, match="bounds_suboptimality"):
        ctx.price_american_bounds_div(pairs[0][0], Q, divs, suboptimality_check="european", **kw)
    assert (ctx._bounds_check, ctx._bounds_every, ctx._bounds_cv) == (0, 0, 0)  # the method put its option back
    for p, m in pairs:
        ctx.price_american_bounds_div(p, Q, divs, exercise_every=3, **kw)
        ctx.price_american_bounds_div(p, Q, divs, suboptimality_check="payoff", **kw)
        _same_bits(ctx.price_american_bounds_div(p, Q, divs, **kw), before[m])  # a plain call returns its old bits


# ---------------------------------------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize("model", dc.MODELS)
def test_deterministic_and_table_fallback(ctx, model):
    p = _params(model, N=13, M=4000)
    divs = _divs(13)
    kw = dict(n_lower=10_000, n_outer=64, n_inner=200, want_q=True, want_samples=True)
    a = ctx.price_american_bounds_div(p, Q, divs, **kw)
    b = ctx.price_american_bounds_div(p, Q, divs, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # every other step decided by the float64 rule: the same decisions
    try:
        c = ctx.price_american_bounds_div(p, Q, divs, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(b, a)
    _same_bits(c, a)
    ctx.price_american_div(p, Q, _divs(13, [(3, 5.0, "cash")]))  # (another schedule through the context's table in between)
    _same_bits(ctx.price_american_bounds_div(p, Q, divs, **kw), a)
    fresh = _ffi.Context(0)
    try:
        _same_bits(fresh.price_american_bounds_div(p, Q, divs, **kw), a)  # and on a context that has seen nothing else
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------- 9. interfaces
def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_bounds_dividends

    kw = dict(n_lower=20_000, n_outer=64, n_inner=64)
    divs = _divs(13)
    for model, m in (("GBM", "gbm"), ("Heston", "heston1")):
        f = price_american_bounds_dividends(100.0, K, R, SIG, T, 4000, 13, dividend_yield=Q, dividends=divs, model=model,
                                            heston_params=dc.HP, heston_scheme="full_truncation", seed=42, stream=5, ctx=ctx,
                                            **kw)
        d = ctx.price_american_bounds_div(_params(m, N=13, M=4000, stream=5, hp=dc.HP), Q, divs, **kw)
        assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                                  d["se_upper"], d["inner_path_steps"])
        np.testing.assert_array_equal(f.betas, d["betas"])
        assert f.policy == "textbook" and set(f.timings_ms) == {"fit", "lower", "upper", "total"}
        assert (f.dividend_yield, f.n_div_steps, f.first_div_step, f.model) == (Q, 3, 1, model.lower())
        assert f.lower - 4 * f.se_lower <= f.upper + 4 * f.se_upper
    s = price_american_bounds_dividends(100.0, K, R, SIG, T, 4000, 13, dividends=divs, exercise_every=4, ctx=ctx, **kw)
    assert s.exercise_every == 4 and s.n_exercise_dates == 4 and np.count_nonzero(s.betas[:, 3]) <= 3
    k = price_american_bounds_dividends(100.0, K, R, SIG, T, 4000, 13, dividends=divs, suboptimality_check="payoff", ctx=ctx,
                                        **kw)
    assert k.suboptimality_check == "payoff" and ctx._bounds_check == 0
    none = price_american_bounds_dividends(100.0, K, R, SIG, T, 4000, 13, ctx=ctx, **kw)
    assert (none.n_div_steps, none.first_div_step) == (0, 0)


def test_c_example_prints_the_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_dividend_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_dividend_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    divs = [(0.125 + 0.25 * i, 1.5, "cash") for i in range(4)]
    for heston, m in ((0, "gbm"), (1, "heston0")):
        out = subprocess.run([str(exe), "20", "20000", "64", "64", str(heston), "1.5"], check=True, capture_output=True,
                             text=True, timeout=300).stdout
        ref = ctx.price_american_bounds_div(_params(m, is_put=False, N=20, M=100_000, hp=dc.HP), 0.0, divs, n_lower=20_000,
                                            n_outer=64, n_inner=64)
        lo, up = (float(v) for v in re.search(r"bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
        assert re.search(r"inner path-steps \d+", out) and "kernels:" in out and "two-pass quote" in out
        assert "4 dividend steps, the first at step 3" in out and not math.isnan(lo)

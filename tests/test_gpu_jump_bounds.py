"""Andersen-Broadie price bounds under jump-diffusion (omc_price_american_bounds_jump, omc_jump_paths_f32;
options_model_amd/csrc/omc_jump_bounds.hip).

The generator against omc_price_american_jump's kept matrix (bits), with and without the variance state, against
omc_heston_paths_sv_f32 where the jumps have size zero, and restarted from its own state; the device's Q^_t, samples, bounds
and counts against the numpy restatements of tests/helpers/bounds_ref.py, bounds_schedule_ref.py and bounds_check_ref.py on
the device's own spots (tests/helpers/jump_bounds_case.py; tests/test_gpu_jump_bounds_fuzz.py runs the same comparison over
random shapes); the degenerate laws against the jump-free bounds, bit for bit; Merton's series; the refusals; determinism;
the facade and the C example.  Every case at a small shape."""
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
from helpers import jump_bounds_case as jc
from helpers import jump_ref as jr
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
JUMP, Q = (1.5, -0.1, 0.15), 0.03
OUT_KEYS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
            "inner_path_steps")


def _params(model="gbm", is_put=True, S0=100.0, N=8, M=2000, seed=42, stream=0, hp=None):
    hp = hp or (jc.HP_CLAMP if model == "heston1" else jc.HP)  # scheme 1 with the Feller-violating set
    return jc.make_params(model, is_put=is_put, S0=S0, K=K, r=R, sigma=SIG, T=T, N=N, M=M, seed=seed, stream=stream, hp=hp)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, keys=OUT_KEYS, arrays=("betas", "q", "samples")):
    for key in keys:
        assert a[key] == b[key], key
    for key in arrays:
        if key in a or key in b:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _plain(ctx, p, **kw):
    """the jump-free bounds call of p's model"""
    return bs.price(ctx, p, **kw)


# ---------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize("model", jc.MODELS)
@pytest.mark.parametrize("M,N", [(4096, 13), (1000, 9), (10, 3), (2, 1)])
def test_generator_is_the_pricing_calls_matrix_with_and_without_the_variance(ctx, model, M, N):
    p = jc.with_(_params(model, N=N, M=M, seed=9, stream=5), pair_offset=3)
    JUMP = (min(1.5, 0.9 * N / T), -0.1, 0.15)  # (lambda T / N may not exceed 1)
    keep = ctx.empty((N + 1, M), np.float32)
    ctx.price_american_jump(p, JUMP, Q, S_keep=keep)
    ref = jc.host(keep)
    S = jc.host(ctx.jump_paths(p, JUMP, Q))
    np.testing.assert_array_equal(_bits(S), _bits(ref))
    assert np.any(S != jc.host(ctx.jump_paths(p, (0.0, 0.0, 0.0), Q)))  # (the jumps are there)
    if jc.is_heston(p):
        Sd, Vd = ctx.jump_paths(p, JUMP, Q, want_v=True)
        S2, V = jc.host(Sd), jc.host(Vd)
        np.testing.assert_array_equal(_bits(S2), _bits(ref))
        assert V.shape == S.shape and np.all(V[0] == np.float32(p.v0)) and np.all(np.isfinite(V))
        # a jump leaves the variance alone: the state is the jump-free generator's at the same drift rate
        _, _, rj = _ffi.jump_table(p, JUMP, Q)
        Sv, Vv = ctx.heston_paths_sv(M, N, p.S0, rj, p.T, *jc.hc.hp_of(p), p.seed, p.stream, p.pair_offset, int(p.heston_scheme))
        Sv.free()
        np.testing.assert_array_equal(_bits(V), _bits(jc.host(Vv)))


@pytest.mark.parametrize("model", ["heston0", "heston1"])
@pytest.mark.parametrize("lam", [0.0, 4.0])
def test_jumps_of_size_zero_keep_the_sv_generators_bits(ctx, model, lam):
    """lambda T / N = 0.5 with mu_j = sigma_j = 0, and lambda = 0: S and V of omc_heston_paths_sv_f32 at rate r - q"""
    M, N = 1000, 8
    p = jc.with_(_params(model, N=N, M=M, seed=11, stream=2), pair_offset=17)
    Sd, Vd = ctx.jump_paths(p, (lam, 0.0, 0.0), Q, want_v=True)
    Sr, Vr = ctx.heston_paths_sv(M, N, p.S0, p.r - Q, p.T, *jc.hc.hp_of(p), p.seed, p.stream, p.pair_offset, int(p.heston_scheme))
    np.testing.assert_array_equal(_bits(jc.host(Sd)), _bits(jc.host(Sr)))
    np.testing.assert_array_equal(_bits(jc.host(Vd)), _bits(jc.host(Vr)))


def test_no_jumps_write_the_vanilla_gbm_matrix(ctx):
    M, N = 1000, 9
    p = jc.with_(_params("gbm", N=N, M=M, seed=11, stream=2), pair_offset=17)
    ref = jc.host(ctx.gbm_paths(M, N, p.S0, p.r - Q, p.sigma, p.T, p.seed, p.stream, p.pair_offset))
    for jump in ((0.0, -0.1, 0.15), (4.5, 0.0, 0.0)):
        np.testing.assert_array_equal(_bits(jc.host(ctx.jump_paths(p, jump, Q))), _bits(ref))


@pytest.mark.parametrize("model", ["heston0", "heston1"])
def test_a_stored_state_is_a_start_state(ctx, model):
    """A restart is a new path from step 1 of its own draws, so only its row 0 is compared: (S[t, j], V[t, j]) -- under scheme 1
    with the Feller-violating set some of them negative -- come back as the start of both partners, not validated, not floored."""
    M, N, off = 1000, 13, 7
    P = M // 2
    p = jc.with_(_params(model, N=N, M=M, stream=5), pair_offset=off)
    Sd, Vd = ctx.jump_paths(p, JUMP, Q, want_v=True)
    S, V = jc.host(Sd), jc.host(Vd)
    if model == "heston1":
        assert V.min() < 0.0
    else:
        assert V.min() >= 0.0
    for t in (0, 4, 12):
        low = np.argsort(np.minimum(V[t, :P], V[t, P:]))[:3]  # the pairs with the lowest variance state at t
        for j in sorted({0, P - 1, *[int(x) for x in low]}):
            for col in (j, j + P):
                g = jc.with_(p, n_paths=2, S0=float(S[t, col]), v0=float(V[t, col]), pair_offset=off + j)
                Xd, Wd = ctx.jump_paths(g, JUMP, Q, want_v=True)
                X, W = jc.host(Xd), jc.host(Wd)
                assert np.all(_bits(X[0]) == _bits(S[t, col:col + 1])) and np.all(_bits(W[0]) == _bits(V[t, col:col + 1]))
                assert X.shape == (N + 1, 2) and np.all(np.isfinite(X)) and np.all(X > 0)


# ---------------------------------------------------------------------------------------------- 2. the restatement
def _run_case(ctx, c, **kw):
    p, jump = jc.case_params(c), jc.jump_of(c)
    given = jc.given_table(ctx, p, jump, c["q"], c["holes"]) if c["policy"] == "given" else None
    ctx.set_option("pass2_tables_irregular_every", c["irr_every"])
    try:
        d = ctx.price_american_bounds_jump(p, jump, c["q"], policy=c["policy"], n_lower=c["n_lower"], n_outer=c["n_outer"],
                                           n_inner=c["n_inner"], betas=given, want_q=True, want_samples=True, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    return p, jump, given, d


@pytest.mark.parametrize("c", jc.DIRECTED, ids=[jc.case_id(c) for c in jc.DIRECTED])
def test_device_equals_restatement(ctx, c):
    p, jump, given, d = _run_case(ctx, c)
    if given is not None:
        np.testing.assert_array_equal(d["betas"], given)
    else:  # omc_lsm_poly's fits on the jump paths of p
        np.testing.assert_array_equal(d["betas"], jc.fitted_table(ctx, p, jump, c["q"], c["policy"]))
    sp = jc.device_spots(ctx, p, jump, c["q"], c["n_lower"], c["n_outer"], c["n_inner"])
    jc.check_against_restatement(p, d, sp, c["n_lower"], c["n_outer"], c["n_inner"])
    vmin = "" if sp["Vo"] is None else f", lowest outer variance state {sp['Vo'].min():.4f}"
    print(f"{jc.case_id(c)}: bounds [{d['lower']:.4f}, {d['upper']:.4f}], inner steps {d['inner_path_steps']}{vmin}")


# ---------------------------------------------------------------------------------------------- 3. an exercise schedule
@pytest.mark.parametrize("model", jc.MODELS)
@pytest.mark.parametrize("k", [2, 3, 9, 14])
def test_schedule_equals_restatement_and_the_masked_call(ctx, model, k):
    N, n_lower, n_outer, n_inner = 9, 1000, 6, 130
    is_put = k != 3
    p = _params(model, is_put=is_put, N=N, S0=100.0 if is_put else 104.0)
    policy = {2: "textbook", 3: "two_pass", 9: "reference", 14: "textbook"}[k]
    kw = dict(n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True)
    d = ctx.price_american_bounds_jump(p, JUMP, Q, policy=policy, exercise_every=k, **kw)
    assert ctx._bounds_every == 0
    np.testing.assert_array_equal(d["betas"], jc.fitted_table(ctx, p, JUMP, Q, policy, k))
    taus = bs.schedule(N, k)
    sp = jc.device_spots(ctx, p, JUMP, Q, n_lower, n_outer, n_inner, ts=taus[:-1])
    bs.check_against_restatement(p, d, sp, k, n_lower, n_outer, n_inner)
    # the all-dates call given the scheduled table (zero rows off the schedule): the same stops, the same Q^ where both have one
    A = ctx.price_american_bounds_jump(p, JUMP, Q, policy="given", betas=d["betas"], **kw)
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
    JUMP = (min(1.5, 0.9 * N / T), -0.1, 0.15)  # (lambda T / N may not exceed 1)
    kw = dict(policy="textbook", n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True)
    dense = ctx.price_american_bounds_jump(p, JUMP, Q, **kw)
    got = ctx.price_american_bounds_jump(p, JUMP, Q, suboptimality_check="payoff", **kw)
    assert ctx._bounds_check == 0
    sp = jc.device_spots(ctx, p, JUMP, Q, n_lower, n_outer, n_inner)
    jc.check_against_restatement(p, dense, sp, n_lower, n_outer, n_inner)
    st = bk.item_steps(sp["So"], sp["inner"], range(n_outer), K, R, T, is_put, dense["betas"])
    assert st["ties"] == 0
    kp = bk.check_against_dense(p, dense, got, 1, sp["So"], None, st["steps"])
    up = bk.upper_bound(sp["So"], sp["inner"], 1, K, R, T, is_put, got["betas"])
    assert up["ties"] == 0 and got["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(got["q"], up["q"], rtol=1e-12, atol=1e-12 * K)
    # upper_checked <= upper up to the walk's rounding (tests/test_gpu_bounds_check.py's tolerance)
    assert np.all(got["samples"] <= dense["samples"] + br.samples_atol(N, dense["q"], K) + bk.WALK_RTOL * K)
    assert got["upper"] <= dense["upper"] + br.samples_atol(N, dense["q"], K) + bk.WALK_RTOL * K
    print(f"{model} N={N}: items kept {kp.mean():.3f}, upper {got['upper']:.6f} (dense {dense['upper']:.6f})")


# ---------------------------------------------------------------------------------------------- 5. the degenerate laws
@pytest.mark.parametrize("model", jc.MODELS)
@pytest.mark.parametrize("jump", [(4.5, 0.0, 0.0), (0.0, -0.1, 0.15)], ids=["zero-size", "no-jumps"])
def test_degenerate_laws_carry_the_jump_free_bits(ctx, model, jump):
    """q = 0 with mu_j = sigma_j = 0 at lambda T / N = 0.5 -- the jump branch runs, with work to do, and changes no bit -- and
    with lambda = 0: every output of the jump-free bounds call, the schedule and the payoff check included"""
    N = 9
    p = _params(model, N=N)
    for kw in (dict(policy="textbook"), dict(policy="two_pass", exercise_every=3),
               dict(policy="reference", suboptimality_check="payoff")):
        kw.update(n_lower=1000, n_outer=40, n_inner=130, want_q=True, want_samples=True)
        a = ctx.price_american_bounds_jump(p, jump, 0.0, **kw)
        b = _plain(ctx, p, **kw)
        _same_bits(a, b)
        assert a["inner_path_steps"] > 0
    c = jc.with_(p, is_put=0)
    given = jc.given_table(ctx, c, jump, 0.0, [t % 3 == 1 for t in range(N + 1)])
    kw = dict(policy="given", betas=given, n_lower=1000, n_outer=6, n_inner=200, want_q=True, want_samples=True)
    _same_bits(ctx.price_american_bounds_jump(c, jump, 0.0, **kw), _plain(ctx, c, **kw))


# ---------------------------------------------------------------------------------------------- 6. a known answer
@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("q", [0.0, 0.03])
def test_never_exercising_policy_gives_mertons_series(ctx, is_put, q):
    """a table of n = 0 rows never stops before N: lower is the European Monte-Carlo value, and the stepwise compound-Poisson
    law is exact (the mass beyond 16 jumps a step is below 1e-14)"""
    N, lam, mu, sj = 8, 1.0, -0.1, 0.15
    p = _params("gbm", is_put=is_put, N=N, seed=1234)
    d = ctx.price_american_bounds_jump(p, (lam, mu, sj), q, policy="given", betas=np.zeros((N + 1, 4)), n_lower=200_000,
                                       n_outer=2, n_inner=2)
    ref = jr.merton(100.0, K, R, q, SIG, T, lam, mu, sj, is_put)
    print(f"put={is_put} q={q}: lower {d['lower']:.5f} +- {d['se_lower']:.5f}, Merton {ref:.5f}")
    assert d["n_exercised_lower"] == 0
    assert abs(d["lower"] - ref) <= 4 * d["se_lower"], (d["lower"], d["se_lower"], ref)


# ---------------------------------------------------------------------------------------------- 7. refusals
SENTINEL = 0xAB


def _raw(ctx, p, jump=JUMP, q=Q, policy=1, regressors=0, n_lower=1000, n_outer=6, n_inner=64, betas=None, null=()):
    """the C call with sentinel-filled outputs -> (rc, outputs untouched?)"""
    N = int(p.n_steps)
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    C.memset(C.byref(out), SENTINEL, C.sizeof(out))
    bo, qo, so = (np.full(shape, np.nan) for shape in ((N + 1, 4), (max(n_outer, 1), N), (max(n_outer, 1),)))
    j = None if "jump" in null else C.byref(_ffi.make_jump(jump))
    b = None if betas is None else np.ascontiguousarray(betas, np.float64)
    rc = ctx.lib.omc_price_american_bounds_jump(ctx.handle, C.byref(p), j, float(q), None if "cfg" in null else C.byref(cfg),
                                                b.ctypes.data if b is not None else None, bo.ctypes.data, qo.ctypes.data,
                                                so.ctypes.data, None if "out" in null else C.byref(out))
    untouched = bytes(out) == bytes([SENTINEL]) * C.sizeof(out) and all(np.isnan(a).all() for a in (bo, qo, so))
    return rc, untouched


def test_refusals_leave_the_outputs_alone(ctx):
    p = _params("gbm")
    h = _params("heston0")
    nan, inf = float("nan"), float("inf")
    cases = [(dict(null=("cfg",)), -7), (dict(null=("out",)), -7), (dict(null=("jump",)), -25), (dict(q=nan), -17),
             (dict(jump=(-1.0, 0.0, 0.1)), -26), (dict(jump=(inf, 0.0, 0.1)), -26), (dict(jump=(1.0, nan, 0.1)), -27),
             (dict(jump=(1.0, 0.0, -0.1)), -27), (dict(jump=(8.5, 0.0, 0.1)), -28), (dict(regressors=1), -4),
             (dict(policy=7), -4), (dict(policy=3), -7), (dict(n_inner=63), -3), (dict(n_outer=7), -3), (dict(n_lower=999), -3)]
    for kw, code in cases:
        for pp in (p, h):
            rc, untouched = _raw(ctx, pp, **kw)
            assert rc == code and untouched, (kw, rc)
    assert _raw(ctx, jc.with_(p, antithetic=0))[0] == -24
    assert _raw(ctx, jc.with_(p, sigma=0.0))[0] == -5
    for scheme in (2, 3):
        rc, untouched = _raw(ctx, jc.with_(h, heston_scheme=scheme))
        assert rc == -12 and untouched
    assert _raw(ctx, _params("gbm", N=252), n_outer=1 << 14, n_inner=1 << 12) == (-16, True)
    assert _raw(ctx, jc.with_(p, semantics=0))[0] == 0  # p->semantics is not used
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _raw(hooked, p) == (-10, True)
    finally:
        hooked.close()


def test_option_refusals_and_the_way_back(ctx):
    kw = dict(n_lower=1000, n_outer=6, n_inner=64, want_q=True, want_samples=True)
    pairs = [(_params(m), m) for m in jc.MODELS]
    before = {m: ctx.price_american_bounds_jump(p, JUMP, Q, **kw) for p, m in pairs}
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
            assert _raw(ctx, jc.with_(p, n_paths=0)) == (-3, True)
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
        ctx.price_american_bounds_jump(pairs[0][0], JUMP, Q, suboptimality_check="european", **kw)
    assert (ctx._bounds_check, ctx._bounds_every, ctx._bounds_cv) == (0, 0, 0)  # the method put its option back
    for p, m in pairs:
        ctx.price_american_bounds_jump(p, JUMP, Q, exercise_every=3, **kw)
        ctx.price_american_bounds_jump(p, JUMP, Q, suboptimality_check="payoff", **kw)
        _same_bits(ctx.price_american_bounds_jump(p, JUMP, Q, **kw), before[m])  # a plain call returns its old bits


def test_generator_refusals(ctx):
    lib, hnd = ctx.lib, ctx.handle
    S, V = ctx.empty((4, 10), np.float32), ctx.empty((4, 10), np.float32)
    g, h = _params("gbm", N=3, M=10), _params("heston1", N=3, M=10)
    j = C.byref(_ffi.make_jump(JUMP))
    try:
        call = lambda p, jj=j, q=Q, s=S.ptr, v=None, ld=10: lib.omc_jump_paths_f32(hnd, C.byref(p), jj, float(q), s, v, ld)  # noqa: E731
        assert call(g) == 0 and call(h) == 0 and call(h, v=V.ptr) == 0
        assert call(g, v=V.ptr) == -7  # a variance matrix under GBM
        assert call(g, s=None) == -7 and call(g, ld=9) == -6 and call(g, jj=None) == -25 and call(g, q=float("nan")) == -17
        assert call(jc.with_(g, n_paths=9)) == -3 and call(jc.with_(g, antithetic=0)) == -24
        assert call(g, jj=C.byref(_ffi.make_jump((3.5, 0.0, 0.1)))) == -28
        assert call(g, jj=C.byref(_ffi.make_jump((-1.0, 0.0, 0.1)))) == -26
        assert call(g, jj=C.byref(_ffi.make_jump((1.0, 0.0, -0.1)))) == -27
        assert call(jc.with_(g, semantics=0)) == 0  # the semantics are not used
        # v0 is a start state under schemes 0 .. 2; QE keeps its check
        for scheme in (0, 1, 2):
            assert call(jc.with_(h, heston_scheme=scheme, v0=-0.01), v=V.ptr) == 0
        qe = jc.with_(h, heston_scheme=3, xi=1.0)
        assert call(qe, v=V.ptr) == 0 and call(jc.with_(qe, v0=-0.01)) == -5
        assert call(jc.with_(h, heston_scheme=4)) == -4
    finally:
        S.free()
        V.free()


# ---------------------------------------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize("model", jc.MODELS)
def test_deterministic_and_table_fallback(ctx, model):
    p = _params(model, N=13, M=4000)
    kw = dict(n_lower=10_000, n_outer=64, n_inner=200, want_q=True, want_samples=True)
    a = ctx.price_american_bounds_jump(p, JUMP, Q, **kw)
    b = ctx.price_american_bounds_jump(p, JUMP, Q, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # every other step decided by the float64 rule: the same decisions
    try:
        c = ctx.price_american_bounds_jump(p, JUMP, Q, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(b, a)
    _same_bits(c, a)
    fresh = _ffi.Context(0)
    try:
        _same_bits(fresh.price_american_bounds_jump(p, JUMP, Q, **kw), a)  # and on a context that has seen nothing else
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------- 9. interfaces
def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_bounds_jumps

    kw = dict(n_lower=20_000, n_outer=64, n_inner=64)
    lam, mu, sj = JUMP
    for model, m in (("GBM", "gbm"), ("Heston", "heston1")):
        f = price_american_bounds_jumps(100.0, K, R, SIG, T, 4000, 13, lam, mu, sj, dividend_yield=Q, model=model,
                                        heston_params=jc.HP, heston_scheme="full_truncation", seed=42, stream=5, ctx=ctx, **kw)
        d = ctx.price_american_bounds_jump(_params(m, N=13, M=4000, stream=5, hp=jc.HP), JUMP, Q, **kw)
        assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                                  d["se_upper"], d["inner_path_steps"])
        np.testing.assert_array_equal(f.betas, d["betas"])
        assert f.policy == "textbook" and set(f.timings_ms) == {"fit", "lower", "upper", "total"}
        assert (f.jump_intensity, f.jump_mean, f.jump_vol, f.dividend_yield, f.model) == (lam, mu, sj, Q, model.lower())
        assert f.lower - 4 * f.se_lower <= f.upper + 4 * f.se_upper
    s = price_american_bounds_jumps(100.0, K, R, SIG, T, 4000, 13, lam, mu, sj, exercise_every=4, ctx=ctx, **kw)
    assert s.exercise_every == 4 and s.n_exercise_dates == 4 and np.count_nonzero(s.betas[:, 3]) <= 3
    k = price_american_bounds_jumps(100.0, K, R, SIG, T, 4000, 13, lam, mu, sj, suboptimality_check="payoff", ctx=ctx, **kw)
    assert k.suboptimality_check == "payoff" and ctx._bounds_check == 0


def test_c_example_prints_the_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_jump_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_jump_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    for bates, m in ((0, "gbm"), (1, "heston0")):
        out = subprocess.run([str(exe), "20", "20000", "64", "64", str(bates), "2.0"], check=True, capture_output=True,
                             text=True, timeout=300).stdout
        ref = ctx.price_american_bounds_jump(_params(m, N=20, M=100_000, hp=jc.HP), (2.0, -0.1, 0.15), 0.0, n_lower=20_000,
                                             n_outer=64, n_inner=64)
        lo, up = (float(v) for v in re.search(r"bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
        assert re.search(r"inner path-steps \d+", out) and "kernels:" in out and "two-pass quote" in out
        assert not math.isnan(lo)

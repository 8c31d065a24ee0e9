"""Price bounds of a game with an exercise schedule (option "bounds_exercise_every"; omc_bounds_sched_dev.h, DESIGN.md
section 25), GBM and Heston with a policy on the spot.

The option's values and its defaults' bits; the all-dates kernels on a policy holed to the schedule against the scheduled
kernels (lower bound and Q^ bit for bit); the numpy restatement of tests/helpers/bounds_schedule_ref.py on the device's own
spots; the fits on the gathered matrix against omc_lsm_poly; the exact inner work of a never-exercising table; known answers
(the lattice of the N / k-date game, Black-Scholes with the expiry alone, xi = 0); a call of two inner launches; determinism;
the refusals; the facades and the C example.  Every case at a small shape."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs
from helpers import call_catalogue as cat
from helpers import heston_bounds_case as hc
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
MODELS = ("gbm", "heston0", "heston1")
TINY = dict(n_lower=4096, n_outer=64, n_inner=64)
OUT_KEYS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
            "inner_path_steps")


def _params(model="gbm", is_put=True, S0=100.0, N=8, M=4096, stream=0, hp=None):
    if model == "gbm":
        return bs.gbm_params(is_put=is_put, S0=S0, K=K, r=R, sigma=SIG, T=T, N=N, M=M, seed=42, stream=stream)
    scheme = int(model[-1])
    hp = hp or (hc.HP_CLAMP if scheme == 1 else hc.HP)  # scheme 1 with the Feller-violating set
    return hc.make_params(hp, scheme=scheme, is_put=is_put, S0=S0, K=K, r=R, T=T, N=N, M=M, seed=42, stream=stream)


def _same_bits(a, b, keys=OUT_KEYS, arrays=("betas", "q", "samples")):
    for key in keys:
        assert a[key] == b[key], key
    for key in arrays:
        if key in a or key in b:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ---------------------------------------------------------------------------------------------- 1. the option
def test_option_values(ctx):
    lib, h = ctx.lib, ctx.handle
    try:
        for k in (0, 1, 2, 5, 2 ** 31 - 1):
            assert lib.omc_set_option(h, b"bounds_exercise_every", k) == 0
        assert lib.omc_set_option(h, b"bounds_exercise_every", 3) == 0
        assert lib.omc_set_option(h, b"bounds_exercise_every", -1) == -4
        assert lib.omc_set_option(h, b"bounds_exercise_every", 2 ** 31) == -4
        # the refused values left the 3: a scheduled call, not the all-dates one
        held = ctx.price_american_bounds(_params(N=7), exercise_every=None, **TINY)  # None: the option as the context holds it
        three = ctx.price_american_bounds(_params(N=7), exercise_every=3, **TINY)
        _same_bits(held, three, arrays=("betas",))
        assert np.all(np.delete(held["betas"], [1, 4, 7], axis=0) == 0.0) and np.count_nonzero(held["betas"][:, 3]) > 0
    finally:
        ctx.set_option("bounds_exercise_every", 0)


@pytest.mark.parametrize("model", MODELS)
def test_every_date_values_keep_the_default_bits(ctx, model):
    p = _params(model, N=7)
    kw = dict(want_q=True, want_samples=True, **TINY)
    fresh = _ffi.Context(0)
    try:
        want = bs.price(fresh, p, exercise_every=None, **kw)  # None: the option is not touched -- this context never set it
    finally:
        fresh.close()
    for k in (0, 1):
        _same_bits(bs.price(ctx, p, exercise_every=k, **kw), want)


# ---------------------------------------------------------------------------------------------- 2. old kernels check the new
def _outer_zmax(ctx, p, n_outer):
    """the largest payoff on the outer paths: the scale of the walk's rounding (bounds_ref.samples_atol)"""
    N = int(p.n_steps)
    if p.model == _ffi.MODELS["gbm"]:
        So = hc.host(ctx.gbm_paths(n_outer, N, p.S0, p.r, p.sigma, p.T, p.seed, p.stream + 2))
    else:
        So = hc.host(ctx.heston_paths(n_outer, N, p.S0, p.r, p.T, *hc.hp_of(p), p.seed, p.stream + 2, 0, int(p.heston_scheme)))
    phi = (K - So) if p.is_put else (So - K)
    return float(max(phi.max(), 0.0))


SHAPES = [(N, k) for N in (7, 8, 12, 13) for k in (2, 3, 5, N - 1, N, N + 3)]
OLD_NEW = [(m, N, k, (64, 66)[(i + j) % 2], (2, 64, 192)[(i + j) % 3], bool(((i + j) // 2) % 2))
           for j, m in enumerate(MODELS) for i, (N, k) in enumerate(SHAPES)]


def test_old_new_cases_cover_the_shapes():
    assert {(c[3], c[4]) for c in OLD_NEW} == {(o, i) for o in (64, 66) for i in (2, 64, 192)}
    assert {(c[1], c[2]) for c in OLD_NEW} == set(SHAPES) and {c[5] for c in OLD_NEW} == {True, False}
    for m in MODELS:
        assert {c[4] for c in OLD_NEW if c[0] == m} == {2, 64, 192} and {c[3] for c in OLD_NEW if c[0] == m} == {64, 66}


@pytest.mark.parametrize("model,N,k,n_outer,n_inner,is_put", OLD_NEW,
                         ids=[f"{c[0]}-N{c[1]}-k{c[2]}-o{c[3]}-i{c[4]}-{'put' if c[5] else 'call'}" for c in OLD_NEW])
def test_all_dates_kernels_on_the_holed_policy(ctx, model, N, k, n_outer, n_inner, is_put):
    """A: the all-dates call given P_k (P with zero rows off the schedule).  B: the scheduled call given P itself."""
    p = _params(model, is_put=is_put, N=N, S0=98.0 if is_put else 102.0)
    P = bs.given_table(ctx, p)
    Pk = bs.mask(P, k)
    kw = dict(policy="given", n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True)
    A = bs.price(ctx, p, betas=Pk, **kw)
    B = bs.price(ctx, p, betas=P, exercise_every=k, **kw)
    np.testing.assert_array_equal(B["betas"], Pk)
    for key in ("lower", "se_lower", "n_exercised_lower"):
        assert B[key] == A[key], key
    taus = bs.schedule(N, k)
    on = taus[:-1]
    off = [t for t in range(N) if t not in on]
    np.testing.assert_array_equal(B["q"][:, on], A["q"][:, on])
    assert np.all(B["q"][:, off] == 0.0)
    atol = br.samples_atol(N, A["q"], _outer_zmax(ctx, p, n_outer))
    assert np.all(B["samples"] <= A["samples"] + atol)
    assert B["inner_path_steps"] <= A["inner_path_steps"]
    assert B["upper"] >= B["lower"] - 4 * (B["se_lower"] + B["se_upper"])


# ---------------------------------------------------------------------------------------------- 5. the exact work
@pytest.mark.parametrize("model,N,k,n_outer,n_inner", [("gbm", 12, 5, 66, 192), ("gbm", 13, 3, 64, 2), ("gbm", 7, 6, 66, 64),
                                                       ("gbm", 8, 11, 64, 192), ("heston0", 13, 5, 66, 64),
                                                       ("heston1", 7, 2, 66, 192), ("heston1", 8, 8, 64, 2)])
def test_a_never_exercising_table_does_the_scheduled_work_exactly(ctx, model, N, k, n_outer, n_inner):
    """an item run at an unscheduled date, or a date missed, changes the count"""
    d = bs.price(ctx, _params(model, N=N), policy="given", betas=np.zeros((N + 1, 4)), n_lower=4096, n_outer=n_outer,
                 n_inner=n_inner, exercise_every=k, want_q=True)
    assert d["inner_path_steps"] == bs.max_inner_steps(N, k, n_outer, n_inner)
    assert d["inner_path_steps"] == n_outer * n_inner * sum(N - t for t in bs.schedule(N, k)[:-1])
    assert d["n_exercised_lower"] == 0
    on = bs.schedule(N, k)[:-1]
    assert np.all(d["q"][:, [t for t in range(N) if t not in on]] == 0.0)


# ---------------------------------------------------------------------------------------------- 3. the restatement
_spots = {}


def _case_spots(ctx, p, model, k, n_lower, n_outer, n_inner):
    """the device's own spots of a case, computed once: they depend on the law and the sizes, not on payoff or policy"""
    key = (model, int(p.n_steps), k, n_lower, n_outer, n_inner)
    if key not in _spots:
        _spots[key] = bs.device_spots(ctx, p, k, n_lower, n_outer, n_inner)
    return _spots[key]


RESTATED = [("gbm", 8, 3, 64, 64, "textbook", True), ("gbm", 8, 3, 64, 64, "given", True), ("gbm", 8, 3, 64, 64, "two_pass", False),
            ("gbm", 8, 3, 64, 64, "reference", True), ("gbm", 7, 5, 16, 192, "textbook", True), ("gbm", 13, 13, 16, 64, "textbook", True),
            ("heston0", 8, 3, 64, 64, "textbook", True), ("heston0", 8, 3, 64, 64, "given", False),
            ("heston1", 7, 2, 16, 192, "textbook", True), ("heston1", 7, 2, 16, 192, "given", True),
            ("heston1", 12, 5, 16, 64, "two_pass", True)]


@pytest.mark.parametrize("model,N,k,n_outer,n_inner,policy,is_put", RESTATED,
                         ids=[f"{c[0]}-N{c[1]}-k{c[2]}-o{c[3]}-i{c[4]}-{c[5]}-{'put' if c[6] else 'call'}" for c in RESTATED])
def test_device_equals_restatement(ctx, model, N, k, n_outer, n_inner, policy, is_put):
    n_lower = 4096
    p = _params(model, is_put=is_put, N=N)
    given = bs.given_table(ctx, p) if policy == "given" else None
    d = bs.price(ctx, p, policy=policy, n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, betas=given, exercise_every=k,
                 want_q=True, want_samples=True)
    if policy == "given":
        np.testing.assert_array_equal(d["betas"], bs.mask(given, k))
    else:
        np.testing.assert_array_equal(d["betas"], bs.fitted_table(ctx, p, policy, k))
    sp = _case_spots(ctx, p, model, k, n_lower, n_outer, n_inner)
    if model == "heston1":
        assert sp["Vo"].min() < 0.0  # inner simulations start at negative variance states too
    bs.check_against_restatement(p, d, sp, k, n_lower, n_outer, n_inner)


# ---------------------------------------------------------------------------------------------- 4. the fits
@pytest.mark.parametrize("policy", ["reference", "textbook", "two_pass"])
@pytest.mark.parametrize("model,N,k,M", [("gbm", 12, 5, 4096), ("gbm", 13, 3, 3002), ("gbm", 8, 8, 4096), ("gbm", 7, 10, 1000),
                                         ("gbm", 12, 4, 4096), ("heston1", 13, 6, 3002), ("heston0", 12, 12, 4096)])
def test_fits_are_lsm_polys_on_the_gathered_matrix(ctx, policy, model, N, k, M):
    p = _params(model, N=N, M=M)
    d = bs.price(ctx, p, policy=policy, n_lower=1000, n_outer=16, n_inner=2, exercise_every=k)
    want = bs.fitted_table(ctx, p, policy, k)  # horizon T_v = T (J k) / N
    np.testing.assert_array_equal(d["betas"], want)
    on = bs.schedule(N, k)[1:]
    assert np.all(np.delete(d["betas"], on, axis=0) == 0.0)
    if bs.n_dates(N, k) > 2:
        assert np.count_nonzero(d["betas"][on[:-1], 3]) > 0  # the scheduled rows do carry fits


# ---------------------------------------------------------------------------------------------- 6. known answers
BIG = dict(n_lower=400_000, n_outer=4096, n_inner=512)  # those of tests/test_gpu_bounds.py


@pytest.mark.parametrize("S0", [90.0, 100.0, 110.0])
def test_brackets_the_lattice_of_the_scheduled_game(ctx, S0):
    """k | N: the scheduled game on the fine GBM paths has the law of the N / k-date game"""
    d = ctx.price_american_bounds(_params(S0=S0, N=48, M=100_000), policy="textbook", exercise_every=4, **BIG)
    V = br.lattice(S0, K, R, SIG, T, 12)
    print(S0, d["lower"], d["se_lower"], d["upper"], d["se_upper"], V, d["inner_path_steps"])
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)
    assert d["upper"] > d["lower"]


@pytest.mark.parametrize("scheme", [0, 1])
def test_heston_without_vol_of_vol_brackets_the_same_lattice(ctx, scheme):
    """xi = 0 and v0 = theta = 0.0625 (exact in float32): the variance stays theta and the law is GBM at sigma = 0.25"""
    hp = dict(hc.HP, v0=0.0625, theta=0.0625, xi=0.0)
    d = ctx.price_american_bounds_heston(_params(f"heston{scheme}", N=48, M=100_000, hp=hp), policy="textbook",
                                         exercise_every=4, **BIG)
    V = br.lattice(100.0, K, R, 0.25, T, 12)
    print(scheme, d["lower"], d["se_lower"], d["upper"], d["se_upper"], V)
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)
    assert d["upper"] > d["lower"]


@pytest.mark.parametrize("is_put,k", [(True, 12), (False, 12), (True, 15)])
def test_the_expiry_alone_is_black_scholes(ctx, is_put, k):
    N = 12
    d = ctx.price_american_bounds(_params(is_put=is_put, N=N, M=4096), exercise_every=k, want_q=True, **BIG)
    bs_ = br.black_scholes(100.0, K, R, SIG, T, is_put)
    assert abs(d["lower"] - bs_) <= 3 * d["se_lower"], (d["lower"], d["se_lower"], bs_)
    assert abs(d["upper"] - bs_) <= 3 * d["se_upper"], (d["upper"], d["se_upper"], bs_)
    assert d["upper"] == pytest.approx(float(np.mean(d["q"][:, 0])), rel=1e-12)  # the sample is Z_N - (Z_N - Q^_0)
    assert d["n_exercised_lower"] == 0 and d["inner_path_steps"] == BIG["n_outer"] * BIG["n_inner"] * N
    assert np.all(d["betas"] == 0.0)


# ---------------------------------------------------------------------------------------------- 7. two inner launches
def test_launch_blocks_restated_on_sampled_outer_paths(ctx):
    """The inner launches split the outer paths by the SCHEDULED worst case n_inner sum_j (N - tau_j): at N = 50, k = 2,
    n_inner = 512 that is 332,800 steps per outer path, blocks of 3226, two launches for 4096.  Q^ of the first, last and a
    middle outer path of either block and of two partner columns against the restatement on the device's own spots, as
    tests/test_gpu_bounds.py does it for the all-dates call."""
    N, k, n_outer, n_inner = 50, 2, 4096, 512
    per_outer = n_inner * sum(N - t for t in bs.schedule(N, k)[:-1])
    blk = (1 << 30) // per_outer
    starts = list(range(0, n_outer, blk))
    assert per_outer == 332_800 and blk == 3226 and len(starts) == 2  # a changed launch rule must not empty this test
    rows = []
    for i0 in starts:
        i1 = min(i0 + blk, n_outer)
        rows += [i0, (i0 + i1) // 2, i1 - 1]
    rows += [n_outer // 2 - 1, n_outer // 2]  # the partner columns of the last and the first outer path: the other block's
    assert len(set(rows)) == len(rows) and 0 <= min(rows) and max(rows) < n_outer
    p = _params(N=N, M=20_000)
    d = ctx.price_american_bounds(p, policy="textbook", n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True,
                                  want_samples=True, exercise_every=k)
    So = hc.host(ctx.gbm_paths(n_outer, N, 100.0, R, SIG, T, 42, 2))
    inner = br.inner_by_item(lambda off, n: hc.host(ctx.gbm_normals(n, N, 42, 3, off)), So, n_inner,
                             lambda z, s0: hc.host(ctx.gbm_paths_from_normals(z, s0, R, SIG, T)))
    qr = bs.q_rows(So, inner, rows, K, R, T, True, d["betas"], k)
    wk = bs.walk_rows(So, qr["q"], rows, K, R, T, True, d["betas"], k)
    print(f"blocks of {blk}: rows {rows}, ties {qr['ties']} + {wk['ties']}")
    assert qr["ties"] == 0 and wk["ties"] == 0  # numpy's decisions are the device's
    np.testing.assert_allclose(d["q"][rows], qr["q"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d["samples"][rows], wk["samples"], rtol=0, atol=br.samples_atol(N, qr["q"], wk["zmax"]))


# ---------------------------------------------------------------------------------------------- 8. determinism
@pytest.mark.parametrize("model", ["gbm", "heston1"])
def test_deterministic_and_table_fallback(ctx, model):
    p = _params(model, N=13, M=20_000)
    kw = dict(n_lower=100_000, n_outer=2048, n_inner=256, want_q=True, want_samples=True, exercise_every=3)
    a = bs.price(ctx, p, **kw)
    b = bs.price(ctx, p, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # every other date decided by the float64 rule: the same decisions
    try:
        c = bs.price(ctx, p, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(b, a)
    _same_bits(c, a)
    assert 0 < a["n_exercised_lower"] < kw["n_lower"]


# ---------------------------------------------------------------------------------------------- 9. refusals
def _cfg(regressors=0, policy=1):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, 1000, 64, 64
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    return cfg


def _unsupported(ctx):
    """name -> (raw call -> (rc, bytes of the output struct), facade call -> result dict) of the four calls that take no schedule"""
    lib, h = ctx.lib, ctx.handle
    ph = _params("heston0")
    pg = _params("gbm")
    pc = _params("gbm", is_put=False)

    def raw(entry, out_t, *head):
        def call():
            out = out_t()
            C.memset(C.byref(out), 0xAB, C.sizeof(out))
            rc = entry(h, *head, None, None, None, None, C.byref(out))
            return rc, bytes(out)
        return call

    small = dict(n_lower=1000, n_outer=64, n_inner=64, want_q=True, want_samples=True)
    asian = _ffi.make_basket([100.0, 95.0], [0.2, 0.3], kind="asian")
    return {
        "heston spot+variance": (raw(lib.omc_price_american_bounds_heston, _ffi.Bounds, C.byref(ph), C.byref(_cfg(1))),
                                 lambda: ctx.price_american_bounds_heston(ph, regressors="spot+variance", exercise_every=None,
                                                                          **small)),
        "basket": (raw(lib.omc_price_american_basket_bounds, _ffi.BasketBounds, C.byref(pg), C.byref(cat.basket3()),
                       C.byref(_cfg())),
                   lambda: ctx.price_american_basket_bounds(pg, cat.basket3(), **small)),
        "asian": (raw(lib.omc_price_american_basket_bounds, _ffi.BasketBounds, C.byref(pg), C.byref(asian), C.byref(_cfg())),
                  lambda: ctx.price_american_basket_bounds(pg, asian, **small)),
        "runner-up": (raw(lib.omc_price_american_basket_bounds_runnerup, _ffi.BasketBounds, C.byref(pc),
                          C.byref(cat.basket3("best-of")), C.byref(_cfg())),
                      lambda: ctx.price_american_basket_bounds(pc, cat.basket3("best-of"), regressors="index+runner-up",
                                                               **small)),
    }


def test_refusals_and_the_way_back(ctx):
    calls = _unsupported(ctx)
    before = {name: facade() for name, (_, facade) in calls.items()}
    pd = _params(N=7)
    default = ctx.price_american_bounds(pd, want_q=True, want_samples=True, **TINY)
    try:
        ctx.set_option("bounds_exercise_every", 2)
        for name, (raw, facade) in calls.items():
            rc, out = raw()
            assert rc == -38 and out == b"\xab" * len(out), name  # refused, the output struct untouched
            assert b"bounds_exercise_every" in ctx.lib.omc_last_error()
            with pytest.raises(ValueError, match="schedule"):
                facade()
        # their own argument checks come first: an odd n_inner is still -3
        cfg = _cfg()
        cfg.n_inner = 63
        out = _ffi.BasketBounds()
        pg = _params("gbm")
        assert ctx.lib.omc_price_american_basket_bounds(ctx.handle, C.byref(pg), C.byref(cat.basket3()), C.byref(cfg), None,
                                                        None, None, None, C.byref(out)) == -3
        # an entry point that computes no bounds ignores the option
        assert ctx.price_american(_params(N=7))["price"] > 0
        ctx.set_option("bounds_exercise_every", 1)  # every date: no refusal
        for name, (raw, _) in calls.items():
            assert raw()[0] == 0, name
        sched = ctx.price_american_bounds(pd, exercise_every=None, want_q=True, want_samples=True, **TINY)  # option 1
        _same_bits(sched, default)
    finally:
        ctx.set_option("bounds_exercise_every", 0)
    for name, (_, facade) in calls.items():
        after = facade()
        assert not cat.diff(cat.flat(after), cat.flat(before[name])), name
    # a default call after a scheduled one
    ctx.price_american_bounds(pd, exercise_every=3, want_q=True, want_samples=True, **TINY)
    _same_bits(ctx.price_american_bounds(pd, want_q=True, want_samples=True, **TINY), default)
    assert ctx._bounds_every == 0


def test_the_context_method_puts_the_option_back(ctx):
    p = _params(N=7)
    try:
        ctx.set_option("bounds_exercise_every", 3)
        three = ctx.price_american_bounds(p, exercise_every=None, **TINY)
        seven = ctx.price_american_bounds(p, exercise_every=7, **TINY)
        assert ctx._bounds_every == 3
        again = ctx.price_american_bounds(p, exercise_every=None, **TINY)
        with pytest.raises(ValueError):
            ctx.price_american_bounds(p, exercise_every=-2, **TINY)
        assert ctx._bounds_every == 3
    finally:
        ctx.set_option("bounds_exercise_every", 0)
    _same_bits(again, three, arrays=("betas",))
    assert seven["inner_path_steps"] == 64 * 64 * 7 and three["inner_path_steps"] != seven["inner_path_steps"]


# ---------------------------------------------------------------------------------------------- 10. facades, example
def test_facades_equal_ffi(ctx):
    from options_model_amd import price_american_bounds, price_american_bounds_heston, price_bermudan_bounds

    kw = dict(n_lower=100_000, n_outer=1024, n_inner=256)
    d = ctx.price_american_bounds(_params(N=12, M=20_000, stream=5), exercise_every=5, **kw)
    for f in (price_american_bounds(100.0, K, R, SIG, T, 20_000, 12, seed=42, stream=5, ctx=ctx, exercise_every=5, **kw),
              price_bermudan_bounds(100.0, K, R, SIG, T, 20_000, 12, 5, seed=42, stream=5, ctx=ctx, **kw)):
        assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                                  d["se_upper"], d["inner_path_steps"])
        np.testing.assert_array_equal(f.betas, d["betas"])
        assert (f.exercise_every, f.n_exercise_dates) == (5, 3)
    every = price_american_bounds(100.0, K, R, SIG, T, 20_000, 12, seed=42, stream=5, ctx=ctx, **kw)
    assert (every.exercise_every, every.n_exercise_dates) == (0, 12) and every.lower > f.lower - 4 * f.se_lower
    ph = hc.make_params(hc.HP, scheme=1, N=12, M=20_000, seed=42, stream=5, K=K, r=R, T=T)
    dh = ctx.price_american_bounds_heston(ph, exercise_every=5, **kw)
    for f in (price_american_bounds_heston(100.0, K, R, T, 20_000, 12, heston_params=hc.HP, heston_scheme="full_truncation",
                                           seed=42, stream=5, ctx=ctx, exercise_every=5, **kw),
              price_bermudan_bounds(100.0, K, R, 0.2, T, 20_000, 12, 5, model="Heston", heston_params=hc.HP,
                                    heston_scheme="full_truncation", seed=42, stream=5, ctx=ctx, **kw)):
        assert (f.lower, f.upper, f.inner_path_steps) == (dh["lower"], dh["upper"], dh["inner_path_steps"])
        assert (f.exercise_every, f.n_exercise_dates, f.regressors) == (5, 3, "spot")
    assert ctx._bounds_every == 0


def test_c_example_prints_the_brackets(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "bermudan_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "bermudan_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    N, k = 48, 4
    out = subprocess.run([str(exe), str(N), str(k), "100000", "1024", "128"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    got = {m[0]: (int(m[1]), int(m[2]), float(m[3]), float(m[4]), int(m[5])) for m in re.findall(
        r"(\w+) put, exercise_every (\d+) \((\d+) dates of 48\): bounds \[([-0-9.]+), ([-0-9.]+)\].*inner path-steps (\d+)", out)}
    assert set(got) == {"american", "bermudan", "european"}, out
    for name, every in (("american", 0), ("bermudan", k), ("european", N)):
        ref = ctx.price_american_bounds(_params(N=N, M=100_000), n_lower=100_000, n_outer=1024, n_inner=128,
                                        exercise_every=every)
        e, dates, lo, up, steps = got[name]
        assert (e, dates, steps) == (every, bs.n_dates(N, every), ref["inner_path_steps"]), (name, out)
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
    assert got["european"][2] < got["bermudan"][2] < got["american"][3]  # European lower < Bermudan lower < American upper

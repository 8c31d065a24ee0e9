"""Sub-optimality checking of the price bounds (option "bounds_suboptimality"; omc_bounds_check_dev.h).

The option's values and its default's bits; every model that takes a check against its own dense call and the numpy
restatement of tests/helpers/bounds_check_ref.py on the device's own outer spots -- the policy and the lower bound bit for
bit, Q^ the dense call's bits at the kept items and 0.0 at the skipped ones, the walk over the kept dates, the kept items'
step count --; every item kept and none kept past date 0; a never-exercising table; one date; a call of two inner launches;
determinism; the statistics against the lattice; the refusals; the facades and the C example.  Every case at a small shape.

Tolerances: what has been through the walk is compared with a float64 walk on the device's own Q^ at
bounds_check_ref.WALK_RTOL = 1e-12 (relative, and in units of K), the tolerance of tests/test_gpu_bounds.py; "at most the dense
sample" adds bounds_ref.samples_atol, the rounding of two walks over the same values."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_check_ref as bk
from helpers import bounds_ref as br
from helpers import call_catalogue as cat
from helpers import heston_bounds_case as hc
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
TINY = dict(n_lower=4096, n_outer=64, n_inner=64)
OUT_KEYS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
            "inner_path_steps")
MODES_OF = {"gbm": (1, 2), "gbm-cv": (1, 2), "basket": (1,), "asian": (1,), "heston1": (1,)}


def _same_bits(a, b, keys=OUT_KEYS, arrays=("betas", "q", "samples")):
    for key in keys:
        assert a[key] == b[key], key
    for key in arrays:
        if key in a or key in b:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _setup(ctx, model, N, is_put, S0, M=4096, policy=None):
    """-> (p, b, the keywords of the policy): textbook fits for a put, a given table that stops early for a call"""
    p, b = bk.params_of(model, is_put=is_put, S0=S0, K=K, r=R, sigma=SIG, T=T, N=N, M=M)
    policy = policy or ("textbook" if is_put else "given")
    return p, b, dict(policy=policy, betas=bk.given_table(ctx, model, p, b) if policy == "given" else None)


# ---------------------------------------------------------------------------------------------- 1. the option
def test_option_values(ctx):
    lib, h = ctx.lib, ctx.handle
    p, b, pol = _setup(ctx, "gbm", 7, True, 100.0)
    try:
        for m in (0, 1, 2):
            assert lib.omc_set_option(h, b"bounds_suboptimality", m) == 0
        for bad in (3, -1, 2 ** 31):
            assert lib.omc_set_option(h, b"bounds_suboptimality", bad) == -4
            assert b"bounds_suboptimality" in lib.omc_last_error()
        # the refused values left the 2: a European-checked call (None: the option as the context holds it)
        held = ctx.price_american_bounds(p, suboptimality_check=None, **TINY)
        on = ctx.price_american_bounds(p, suboptimality_check="european", **TINY)
        _same_bits(held, on, arrays=("betas",))
        assert lib.omc_set_option(h, b"bounds_suboptimality", 0) == 0
        assert lib.omc_set_option(h, b"bounds_suboptimality", 3) == -4
        off = ctx.price_american_bounds(p, suboptimality_check=None, **TINY)
        assert off["inner_path_steps"] > on["inner_path_steps"] and off["lower"] == on["lower"]
    finally:
        lib.omc_set_option(h, b"bounds_suboptimality", 0)
    with pytest.raises(ValueError, match="suboptimality_check"):
        ctx.price_american_bounds(p, suboptimality_check="sometimes", **TINY)
    assert ctx._bounds_check == 0


@pytest.mark.parametrize("model", ["gbm", "gbm-cv", "basket", "asian", "heston1"])
def test_off_is_off(ctx, model):
    p, b, pol = _setup(ctx, model, 7, True, 100.0)
    kw = dict(want_q=True, want_samples=True, **TINY, **pol)
    fresh = _ffi.Context(0)
    try:
        want = bk.call(fresh, model, p, b, None, **kw)  # None: this context never set the key
    finally:
        fresh.close()
    _same_bits(bk.call(ctx, model, p, b, 0, **kw), want)
    bk.call(ctx, model, p, b, 1, **kw)
    _same_bits(bk.call(ctx, model, p, b, None, **kw), want)  # a default call after a checked one
    assert ctx._bounds_check == 0


# ---------------------------------------------------------------------------------------------- 2. against the dense call
# (model, N, n_outer, n_inner, is_put, S0): N in 1, 2, 7, 13; n_outer 64 and 66; n_inner 2, 16, 24, 64, 192 -- under the control
# variate the lane groups G = 8 (2, 16), 16 (24: a ragged group of 12), 32 (64) and 64 (192: the refill) --; S0 in 90, 100, 110
DENSE = [("gbm", 1, 64, 2, True, 100.0), ("gbm", 2, 66, 16, False, 110.0), ("gbm", 7, 64, 24, True, 90.0),
         ("gbm", 13, 66, 64, False, 100.0), ("gbm", 7, 66, 192, True, 110.0),
         ("gbm-cv", 7, 64, 2, True, 100.0), ("gbm-cv", 13, 66, 16, False, 90.0), ("gbm-cv", 7, 64, 24, True, 110.0),
         ("gbm-cv", 2, 66, 64, True, 100.0), ("gbm-cv", 13, 64, 192, True, 90.0),
         ("basket", 7, 64, 64, True, 100.0), ("basket", 13, 66, 2, False, 110.0),
         ("asian", 7, 66, 16, True, 100.0), ("asian", 13, 64, 24, False, 90.0),
         ("heston1", 7, 64, 64, True, 100.0), ("heston1", 13, 66, 16, False, 110.0), ("heston1", 1, 64, 2, True, 90.0)]


def test_dense_cases_cover_the_shapes():
    assert {c[1] for c in DENSE} == {1, 2, 7, 13} and {c[2] for c in DENSE} == {64, 66}
    assert {c[3] for c in DENSE} == {2, 16, 24, 64, 192} and {c[5] for c in DENSE} == {90.0, 100.0, 110.0}
    assert {c[0] for c in DENSE} == set(MODES_OF) and {c[4] for c in DENSE} == {True, False}
    assert {c[3] for c in DENSE if c[0] == "gbm-cv"} == {2, 16, 24, 64, 192}


@pytest.mark.parametrize("model,N,n_outer,n_inner,is_put,S0", DENSE,
                         ids=[f"{c[0]}-N{c[1]}-o{c[2]}-i{c[3]}-{'put' if c[4] else 'call'}-{c[5]:.0f}" for c in DENSE])
def test_checked_call_against_the_dense_call(ctx, model, N, n_outer, n_inner, is_put, S0):
    p, b, pol = _setup(ctx, model, N, is_put, S0)
    kw = dict(n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True, **pol)
    dense = bk.call(ctx, model, p, b, 0, **kw)
    sp = bk.device_spots(ctx, model, p, b, 2, n_outer, n_inner)
    try:
        st = bk.item_steps(sp["So"], sp["inner"], range(n_outer), K, R, T, is_put, dense["betas"])
    finally:
        sp["free"]()
    assert st["ties"] == 0
    kept = {}
    for mode in MODES_OF[model]:
        got = bk.call(ctx, model, p, b, mode, **kw)
        kp = bk.check_against_dense(p, dense, got, mode, sp["So"], SIG, st["steps"])
        kept[mode] = kp
        print(f"{model} N={N} mode {mode}: items kept {kp.mean():.3f}, inner steps kept "
              f"{got['inner_path_steps'] / max(dense['inner_path_steps'], 1):.3f}, upper {got['upper']:.6f} (dense {dense['upper']:.6f})")
        _same_bits(bk.call(ctx, model, p, b, mode, **kw), got)  # identical calls, identical bits
    if len(kept) == 2:
        assert np.all(kept[1][kept[2]])  # the European check keeps a subset of the payoff check's items
    assert ctx._bounds_check == 0


# ---------------------------------------------------------------------------------------------- 3. the edges of the kept set
@pytest.mark.parametrize("model", ["gbm", "gbm-cv", "heston1"])
def test_every_item_kept_gives_the_dense_bits(ctx, model):
    """a put deep in the money keeps every item of the payoff check: the dense call's samples, upper bound and step count"""
    p, b, pol = _setup(ctx, model, 7, True, 50.0, policy="textbook")
    kw = dict(n_lower=4096, n_outer=66, n_inner=24, want_q=True, want_samples=True, **pol)
    So = bk.outer_index(ctx, model, p, b, 66)
    assert bk.keep(So, np.zeros((8, 4)), 1, K, R, T, True)["keep"].all()  # the payoff alone keeps them
    _same_bits(bk.call(ctx, model, p, b, 1, **kw), bk.call(ctx, model, p, b, 0, **kw))


@pytest.mark.parametrize("model", ["gbm", "basket"])
def test_nothing_kept_past_date_zero(ctx, model):
    """a call far out of the money keeps the items of date 0 alone: the walk sees N only, every sample is Q^_0"""
    N, n_outer = 7, 64
    p, b, pol = _setup(ctx, model, N, False, 60.0)
    kw = dict(n_lower=4096, n_outer=n_outer, n_inner=16, want_q=True, want_samples=True, **pol)
    got = bk.call(ctx, model, p, b, 1, **kw)
    So = bk.outer_index(ctx, model, p, b, n_outer)
    kd = bk.keep(So, got["betas"], 1, K, R, T, False)
    assert kd["ties"] == 0 and kd["keep"][0].all() and not kd["keep"][1:].any()
    assert np.all(got["q"][:, 1:] == 0.0)
    assert abs(got["upper"] - float(np.mean(got["q"][:, 0]))) <= 1e-12
    np.testing.assert_allclose(got["samples"], got["q"][:, 0], rtol=0, atol=1e-12)


NEVER = [("gbm", 7, 64, 2, True), ("gbm-cv", 13, 66, 24, True), ("basket", 7, 66, 64, False), ("heston1", 13, 64, 16, True),
         ("asian", 2, 66, 192, True)]


@pytest.mark.parametrize("model,N,n_outer,n_inner,is_put", NEVER, ids=[f"{c[0]}-N{c[1]}-i{c[3]}" for c in NEVER])
def test_a_never_exercising_table(ctx, model, N, n_outer, n_inner, is_put):
    """every inner path runs to expiry: the step count is n_inner sum over the kept items of (N - t), exactly"""
    p, b = bk.params_of(model, is_put=is_put, S0=100.0, K=K, r=R, sigma=SIG, T=T, N=N)
    got = bk.call(ctx, model, p, b, 1, policy="given", betas=np.zeros((N + 1, 4)), n_lower=4096, n_outer=n_outer,
                  n_inner=n_inner, want_q=True)
    So = bk.outer_index(ctx, model, p, b, n_outer)
    kp = bk.keep(So, np.zeros((N + 1, 4)), 1, K, R, T, is_put)["keep"]
    want = n_inner * int(sum((N - t) * int(kp[t].sum()) for t in range(N)))
    assert got["inner_path_steps"] == want and got["n_exercised_lower"] == 0
    assert 0 < kp.sum() and (N == 1 or kp.sum() < kp.size)
    assert np.all(got["q"][~kp.T] == 0.0)


@pytest.mark.parametrize("mode", [1, 2])
def test_one_date(ctx, mode):
    """N = 1: the item of date 0 and the expiry, nothing to skip -- the dense call's bits"""
    p, b, pol = _setup(ctx, "gbm-cv", 1, True, 100.0)
    kw = dict(n_lower=4096, n_outer=66, n_inner=24, want_q=True, want_samples=True, **pol)
    _same_bits(bk.call(ctx, "gbm-cv", p, b, mode, **kw), bk.call(ctx, "gbm-cv", p, b, 0, **kw))


# ---------------------------------------------------------------------------------------------- 4. two launches, determinism
@pytest.mark.parametrize("model", ["gbm", "gbm-cv"])
def test_two_inner_launches(ctx, model):
    """At N = 50, n_inner = 512 the worst case is 652,800 steps per outer path: blocks of 1644, two launches for 2048, each with
    a kept list of its own"""
    N, n_outer, n_inner = 50, 2048, 512
    per_outer = n_inner * N * (N + 1) // 2
    blk = (1 << 30) // per_outer
    assert per_outer == 652_800 and blk == 1644 and len(range(0, n_outer, blk)) == 2  # a changed launch rule must not empty this
    p, b, pol = _setup(ctx, model, N, True, 100.0, M=20_000)
    kw = dict(n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True, want_samples=True, **pol)
    dense = bk.call(ctx, model, p, b, 0, **kw)
    So = bk.outer_index(ctx, model, p, b, n_outer)
    rows = [0, blk // 2, blk - 1, blk, (blk + n_outer) // 2, n_outer - 1, n_outer // 2 - 1, n_outer // 2]  # walked in numpy
    for mode in (1, 2):
        got = bk.call(ctx, model, p, b, mode, **kw)
        kp = bk.check_against_dense(p, dense, got, mode, So, SIG, rows=rows)
        assert kp[:, :blk].sum() < kp[:, :blk].size and kp[:, blk:].sum() < kp[:, blk:].size  # either block skips
        assert kp[1:, :blk].any() and kp[1:, blk:].any()                                       # ... and keeps
        assert got["inner_path_steps"] < dense["inner_path_steps"]


@pytest.mark.parametrize("model,mode", [("gbm", 1), ("gbm-cv", 2), ("heston1", 1), ("asian", 1)])
def test_deterministic_and_table_fallback(ctx, model, mode):
    p, b, pol = _setup(ctx, model, 13, True, 100.0, M=20_000)
    kw = dict(n_lower=100_000, n_outer=1024, n_inner=24, want_q=True, want_samples=True, **pol)
    a = bk.call(ctx, model, p, b, mode, **kw)
    again = bk.call(ctx, model, p, b, mode, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # every other date decided by the float64 rule: the same decisions
    try:
        c = bk.call(ctx, model, p, b, mode, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(again, a)
    _same_bits(c, a)
    assert 0 < a["n_exercised_lower"] < kw["n_lower"] and np.any(a["q"][:, 1:] == 0.0) and np.any(a["q"][:, 1:] != 0.0)


# ---------------------------------------------------------------------------------------------- 5. the statistics
@pytest.mark.parametrize("S0", [90.0, 100.0, 110.0])
@pytest.mark.parametrize("model", ["gbm", "gbm-cv"])
def test_statistics_at_twelve_dates(ctx, model, S0):
    N = 12
    p, b, pol = _setup(ctx, model, N, True, S0, M=100_000, policy="textbook")
    kw = dict(n_lower=400_000, n_outer=2048, n_inner=64, want_q=True, **pol)
    d = [bk.call(ctx, model, p, b, mode, **kw) for mode in (0, 1, 2)]
    V = br.lattice(S0, K, R, SIG, T, N)
    tol = br.samples_atol(N, d[0]["q"], K) + bk.WALK_RTOL * K
    for mode, x in enumerate(d):
        print(f"{model} S0={S0:.0f} mode {mode}: [{x['lower']:.5f}, {x['upper']:.5f}] se {x['se_lower']:.5f} / {x['se_upper']:.5f}  "
              f"steps {x['inner_path_steps'] / d[0]['inner_path_steps']:.3f}  lattice {V:.5f}")
        assert (x["lower"], x["se_lower"], x["n_exercised_lower"]) == (d[0]["lower"], d[0]["se_lower"], d[0]["n_exercised_lower"])
        assert x["ci_lo"] <= V <= x["ci_hi"], (x, V)
    assert d[2]["upper"] <= d[1]["upper"] + tol and d[1]["upper"] <= d[0]["upper"] + tol
    assert d[2]["inner_path_steps"] < d[1]["inner_path_steps"] < d[0]["inner_path_steps"]


# ---------------------------------------------------------------------------------------------- 6. refusals
def _cfg(regressors=0, policy=1):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, 1000, 64, 64
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    return cfg


def _calls(ctx):
    """name -> (raw call -> (rc, bytes of the output struct), facade call -> result dict)"""
    lib, h = ctx.lib, ctx.handle
    ph = hc.make_params(hc.HP, scheme=0, is_put=True, S0=100.0, K=K, r=R, T=T, N=8, M=4096, seed=42, stream=0)
    pg, _ = bk.params_of("gbm", N=8)
    pc, _ = bk.params_of("gbm", is_put=False, N=8)

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
        "gbm": (raw(lib.omc_price_american_bounds, _ffi.Bounds, C.byref(pg), C.byref(_cfg())),
                lambda: ctx.price_american_bounds(pg, **small)),
        "heston spot": (raw(lib.omc_price_american_bounds_heston, _ffi.Bounds, C.byref(ph), C.byref(_cfg(0))),
                        lambda: ctx.price_american_bounds_heston(ph, **small)),
        "heston spot+variance": (raw(lib.omc_price_american_bounds_heston, _ffi.Bounds, C.byref(ph), C.byref(_cfg(1))),
                                 lambda: ctx.price_american_bounds_heston(ph, regressors="spot+variance", **small)),
        "basket": (raw(lib.omc_price_american_basket_bounds, _ffi.BasketBounds, C.byref(pg), C.byref(cat.basket3()),
                       C.byref(_cfg())),
                   lambda: ctx.price_american_basket_bounds(pg, cat.basket3(), **small)),
        "asian": (raw(lib.omc_price_american_basket_bounds, _ffi.BasketBounds, C.byref(pg), C.byref(asian), C.byref(_cfg())),
                  lambda: ctx.price_american_basket_bounds(pg, asian, **small)),
        "runner-up": (raw(lib.omc_price_american_basket_bounds_runnerup, _ffi.BasketBounds, C.byref(pc),
                          C.byref(cat.basket3("best-of")), C.byref(_cfg())),
                      lambda: ctx.price_american_basket_bounds(pc, cat.basket3("best-of"), regressors="index+runner-up",
                                                               **small)),
        "asian index+spot": (raw(lib.omc_price_american_basket_bounds_runnerup, _ffi.BasketBounds, C.byref(pg), C.byref(asian),
                                 C.byref(_cfg())),
                             lambda: ctx.price_american_basket_bounds(pg, asian, regressors="index+spot", **small)),
    }


REFUSED = {1: {"heston spot+variance", "runner-up", "asian index+spot"},
           2: {"heston spot", "heston spot+variance", "basket", "asian", "runner-up", "asian index+spot"}}


def test_refusals_and_the_way_back(ctx):
    calls = _calls(ctx)
    before = {name: facade() for name, (_, facade) in calls.items()}
    pd, _ = bk.params_of("gbm", N=7)
    fresh = _ffi.Context(0)
    try:
        default = fresh.price_american_bounds(pd, want_q=True, want_samples=True, **TINY)
    finally:
        fresh.close()
    try:
        for m in (1, 2):
            ctx.set_option("bounds_suboptimality", m)
            for name, (raw, facade) in calls.items():
                rc, out = raw()
                if name in REFUSED[m]:
                    assert rc == -40 and out == b"\xab" * len(out), (m, name)  # refused, the output struct untouched
                    assert b"bounds_suboptimality" in ctx.lib.omc_last_error()
                    with pytest.raises(ValueError, match="bounds_suboptimality"):
                        facade()
                else:
                    assert rc == 0, (m, name)
        # a schedule with a check: every bounds call is refused, the ones that take no schedule with -38 first
        ctx.set_option("bounds_suboptimality", 1)
        ctx.set_option("bounds_exercise_every", 2)
        assert calls["gbm"][0]()[0] == -40 and calls["heston spot"][0]()[0] == -40
        assert calls["basket"][0]()[0] == -38 and calls["runner-up"][0]()[0] == -38
        ctx.set_option("bounds_exercise_every", 0)
        # ... and -39 comes before -40
        ctx.set_option("bounds_control_variate", 1)
        ctx.set_option("bounds_suboptimality", 2)
        assert calls["heston spot"][0]()[0] == -39 and calls["basket"][0]()[0] == -39 and calls["gbm"][0]()[0] == 0
        ctx.set_option("bounds_control_variate", 0)
        # their own argument checks come first: an odd n_inner is still -3
        cfg = _cfg()
        cfg.n_inner = 63
        out = _ffi.BasketBounds()
        pg, _ = bk.params_of("gbm", N=8)
        assert ctx.lib.omc_price_american_basket_bounds(ctx.handle, C.byref(pg), C.byref(cat.basket3()), C.byref(cfg), None,
                                                        None, None, None, C.byref(out)) == -3
        # an entry point that computes no bounds ignores the option
        assert ctx.price_american(pd)["price"] > 0
    finally:
        ctx.set_option("bounds_exercise_every", 0)
        ctx.set_option("bounds_control_variate", 0)
        ctx.set_option("bounds_suboptimality", 0)
    for name, (raw, facade) in calls.items():
        assert raw()[0] == 0, name
        after = facade()
        assert not cat.diff(cat.flat(after), cat.flat(before[name])), name  # the old bits
    # a default call after a checked one, against a context that never saw the option
    ctx.price_american_bounds(pd, suboptimality_check="european", want_q=True, want_samples=True, **TINY)
    _same_bits(ctx.price_american_bounds(pd, want_q=True, want_samples=True, **TINY), default)
    assert ctx._bounds_check == 0


# ---------------------------------------------------------------------------------------------- 7. the facades, the example
def test_facades(ctx):
    from options_model_amd import price_american_basket_bounds, price_american_bounds_checked

    kw = dict(n_lower=20_000, n_outer=256, n_inner=16)
    p, _ = bk.params_of("gbm", N=12, M=20_000, stream=5)
    for check, cvon in (("european", True), ("payoff", False), ("off", False)):
        d = ctx.price_american_bounds(p, control_variate=cvon, suboptimality_check=check, **kw)
        f = price_american_bounds_checked(100.0, K, R, SIG, T, 20_000, 12, check=check, seed=42, stream=5, ctx=ctx,
                                          control_variate=cvon, **kw)
        assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                                  d["se_upper"], d["inner_path_steps"])
        assert f.suboptimality_check == check and f.control_variate is cvon and f.exercise_every == 0
    ph = hc.make_params(hc.HP, scheme=0, N=12, M=20_000, stream=5)
    dh = ctx.price_american_bounds_heston(ph, suboptimality_check="payoff", **kw)
    fh = price_american_bounds_checked(100.0, K, R, SIG, T, 20_000, 12, check="payoff", model="Heston", heston_params=hc.HP,
                                       seed=42, stream=5, ctx=ctx, **kw)
    assert (fh.lower, fh.upper, fh.inner_path_steps) == (dh["lower"], dh["upper"], dh["inner_path_steps"])
    assert fh.suboptimality_check == "payoff" and fh.regressors == "spot"
    plain = ctx.price_american_bounds_heston(ph, **kw)
    assert plain["inner_path_steps"] > dh["inner_path_steps"] and plain["lower"] == dh["lower"]
    bargs = ([96.0, 103.0], K, R, [0.16, 0.22], T, 20_000, 12)
    fb = price_american_basket_bounds(*bargs, seed=42, ctx=ctx, suboptimality_check="payoff", **kw)
    fb0 = price_american_basket_bounds(*bargs, seed=42, ctx=ctx, **kw)
    assert fb.suboptimality_check == "payoff" and fb0.suboptimality_check == "off"
    assert fb.lower == fb0.lower and fb.inner_path_steps < fb0.inner_path_steps and fb.upper <= fb0.upper + 1e-9
    assert ctx._bounds_check == 0 and ctx._bounds_cv == 0 and ctx._bounds_every == 0


def test_c_example_prints_the_three_brackets(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_bounds_checked"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_bounds_checked.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    N = 12
    out = subprocess.run([str(exe), str(N), "100000", "1024", "16", "1"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    got = {m[0]: (int(m[1]), int(m[2]), float(m[3]), float(m[4]), int(m[5])) for m in re.findall(
        r"check (\w+) put, suboptimality (\d), n_inner (\d+): bounds \[([-0-9.]+), ([-0-9.]+)\].*inner path-steps (\d+)", out)}
    assert set(got) == set(bk.MODES), out
    p, _ = bk.params_of("gbm", N=N, M=100_000)
    for mode, name in enumerate(bk.MODES):
        ref = ctx.price_american_bounds(p, n_lower=100_000, n_outer=1024, n_inner=16, control_variate=True,
                                        suboptimality_check=name)
        v, ni, lo, up, steps = got[name]
        assert (v, ni, steps) == (mode, 16, ref["inner_path_steps"]), (name, out)
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)

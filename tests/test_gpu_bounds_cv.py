"""The Black-Scholes control variate of the GBM price bounds (option "bounds_control_variate"; omc_bounds_cv_dev.h, DESIGN.md
section 26).

The option's values and its defaults' bits; the same stops as the plain call; a never-exercising table, whose every value is
known without an inner path; the numpy restatement of tests/helpers/bounds_cv_ref.py on the device's own spots; the lane
groups; the statistics (smaller standard errors, an upper bound a small n_inner no longer inflates, the lattice inside the
interval); the refusals; a call of two inner launches; determinism; the facades and the C example.  Every case at a small shape.

CV_TOL: the restated cases of this file and of test_gpu_bounds_cv_fuzz.py deviate from the float64 restatement by at most
bounds_cv_ref.MEASURED = 3.6e-16 (units of K, the worst of q and lower) and, for what has been through the walk,
bounds_cv_ref.MEASURED_WALK = 5.4e-16 (the worst of samples and upper); the bounds CV_TOL and CV_TOL_WALK are 4 times those:
1.44e-15 K and 2.16e-15 K.  The device's erfc / log and libm's differ by ulps, and Z - D E
cancels.  Standard errors also get what the device's own E[m^2] - mean^2 loses to cancellation (bounds_cv_ref.se_atol)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_cv_ref as cv
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bs
from helpers import call_catalogue as cat
from helpers import heston_bounds_case as hc
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
CV_TOL = cv.CV_TOL  # 4 times the worst deviation of q and lower measured over the restated cases, units of K (bounds_cv_ref)
CV_TOL_WALK = cv.CV_TOL_WALK  # ... of samples and upper
TINY = dict(n_lower=4096, n_outer=64, n_inner=64)
OUT_KEYS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
            "inner_path_steps")
N_INNER = (2, 16, 24, 64, 66, 192)  # half-counts 1, 8, 12, 32, 33, 96: every G, a ragged group, the refill


def _params(is_put=True, S0=100.0, N=8, M=4096, stream=0):
    return bs.gbm_params(is_put=is_put, S0=S0, K=K, r=R, sigma=SIG, T=T, N=N, M=M, seed=42, stream=stream)


def _same_bits(a, b, keys=OUT_KEYS, arrays=("betas", "q", "samples")):
    for key in keys:
        assert a[key] == b[key], key
    for key in arrays:
        if key in a or key in b:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _given(ctx, p):
    """a table that does stop paths early: the textbook fits of other paths, for a call (never exercised early without
    dividends) with the continuation values scaled down"""
    t = bs.given_table(ctx, p)
    if not p.is_put:
        t[:, :3] *= 0.9
    return t


# ---------------------------------------------------------------------------------------------- 1. the option
def test_option_values(ctx):
    lib, h = ctx.lib, ctx.handle
    p = _params(N=7)
    try:
        assert lib.omc_set_option(h, b"bounds_control_variate", 0) == 0
        assert lib.omc_set_option(h, b"bounds_control_variate", 1) == 0
        for bad in (2, -1, 2 ** 31):
            assert lib.omc_set_option(h, b"bounds_control_variate", bad) == -4
        # the refused values left the 1: a controlled call (None: the option as the context holds it)
        held = ctx.price_american_bounds(p, control_variate=None, **TINY)
        on = ctx.price_american_bounds(p, control_variate=True, **TINY)
        _same_bits(held, on, arrays=("betas",))
        assert lib.omc_set_option(h, b"bounds_control_variate", 0) == 0
        assert lib.omc_set_option(h, b"bounds_control_variate", 2) == -4
        off = ctx.price_american_bounds(p, control_variate=None, **TINY)
        assert off["se_lower"] > on["se_lower"] and off["lower"] != on["lower"]
    finally:
        ctx.set_option("bounds_control_variate", 0)


def test_facade_keyword(ctx):
    from options_model_amd import price_american_bounds, price_bermudan_bounds

    kw = dict(n_lower=20_000, n_outer=256, n_inner=16)
    d = ctx.price_american_bounds(_params(N=12, M=20_000, stream=5), control_variate=True, exercise_every=5, **kw)
    for f in (price_american_bounds(100.0, K, R, SIG, T, 20_000, 12, seed=42, stream=5, ctx=ctx, control_variate=True,
                                    exercise_every=5, **kw),
              price_bermudan_bounds(100.0, K, R, SIG, T, 20_000, 12, 5, seed=42, stream=5, ctx=ctx, control_variate=True, **kw)):
        assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                                  d["se_upper"], d["inner_path_steps"])
        assert f.control_variate is True and (f.exercise_every, f.n_exercise_dates) == (5, 3)
    plain = price_american_bounds(100.0, K, R, SIG, T, 20_000, 12, seed=42, stream=5, ctx=ctx, exercise_every=5, **kw)
    assert plain.control_variate is False and plain.se_lower > d["se_lower"]
    assert plain.inner_path_steps == d["inner_path_steps"] and plain.n_exercised_lower == d["n_exercised_lower"]
    assert ctx._bounds_cv == 0 and ctx._bounds_every == 0


@pytest.mark.parametrize("k", [0, 3])
def test_option_zero_keeps_the_default_bits(ctx, k):
    p = _params(N=7)
    kw = dict(want_q=True, want_samples=True, exercise_every=k, **TINY)
    fresh = _ffi.Context(0)
    try:
        want = fresh.price_american_bounds(p, control_variate=None, **kw)  # None: this context never set the key
    finally:
        fresh.close()
    _same_bits(ctx.price_american_bounds(p, control_variate=False, **kw), want)
    ctx.price_american_bounds(p, control_variate=True, **kw)
    _same_bits(ctx.price_american_bounds(p, **kw), want)  # a default call after a controlled one


# ---------------------------------------------------------------------------------------------- 2. the same stops
SHAPES = [(N, k) for N in (7, 8, 12, 13) for k in (0, 3, N - 1, N + 3)]
STOPS = [(N, k, (64, 66)[i % 2], N_INNER[i % 6], bool((i // 2) % 2), ("textbook", "given", "two_pass", "reference")[(i // 3) % 4])
         for i, (N, k) in enumerate(SHAPES)]


def test_stops_cases_cover_the_shapes():
    assert {c[3] for c in STOPS} == set(N_INNER) and {c[2] for c in STOPS} == {64, 66} and {c[4] for c in STOPS} == {True, False}
    assert {(c[0], c[1]) for c in STOPS} == set(SHAPES) and len({c[5] for c in STOPS}) == 4


@pytest.mark.parametrize("N,k,n_outer,n_inner,is_put,policy", STOPS,
                         ids=[f"N{c[0]}-k{c[1]}-o{c[2]}-i{c[3]}-{'put' if c[4] else 'call'}-{c[5]}" for c in STOPS])
def test_same_stops_as_the_plain_call(ctx, N, k, n_outer, n_inner, is_put, policy):
    p = _params(is_put=is_put, N=N, S0=98.0 if is_put else 102.0)
    kw = dict(policy=policy, betas=_given(ctx, p) if policy == "given" else None, n_lower=4096, n_outer=n_outer,
              n_inner=n_inner, exercise_every=k, want_q=True, want_samples=True)
    plain = ctx.price_american_bounds(p, **kw)
    on = ctx.price_american_bounds(p, control_variate=True, **kw)
    np.testing.assert_array_equal(on["betas"], plain["betas"])
    assert on["n_exercised_lower"] == plain["n_exercised_lower"] and on["inner_path_steps"] == plain["inner_path_steps"]
    off = [t for t in range(N) if t not in bs.schedule(N, k)[:-1]]
    assert np.all(on["q"][:, off] == 0.0) and np.all(np.isfinite(on["q"])) and np.all(np.isfinite(on["samples"]))
    assert on["se_lower"] <= plain["se_lower"]
    assert abs(on["lower"] - plain["lower"]) <= 5 * plain["se_lower"] + 1e-12 * K
    _same_bits(ctx.price_american_bounds(p, control_variate=True, **kw), on)  # identical calls, identical bits


# ---------------------------------------------------------------------------------------------- 3. a never-exercising table
NEVER = [(7, 0, 64, 2, True), (8, 3, 66, 16, False), (12, 11, 64, 24, True), (13, 16, 66, 64, False), (8, 0, 66, 66, False),
         (12, 3, 64, 192, True), (7, 10, 66, 16, True), (13, 0, 64, 192, False)]


@pytest.mark.parametrize("N,k,n_outer,n_inner,is_put", NEVER,
                         ids=[f"N{c[0]}-k{c[1]}-o{c[2]}-i{c[3]}-{'put' if c[4] else 'call'}" for c in NEVER])
def test_a_never_exercising_table(ctx, N, k, n_outer, n_inner, is_put):
    """every partner runs to expiry and contributes exactly 0: all values are known without an inner path"""
    p = _params(is_put=is_put, N=N)
    d = ctx.price_american_bounds(p, policy="given", betas=np.zeros((N + 1, 4)), n_lower=4096, n_outer=n_outer, n_inner=n_inner,
                                  exercise_every=k, control_variate=True, want_q=True, want_samples=True)
    E0 = cv.e0(100.0, N, K, R, SIG, T, is_put)
    assert abs(d["lower"] - E0) <= 1e-13 * E0 and d["se_lower"] == 0.0 and d["n_exercised_lower"] == 0
    assert d["inner_path_steps"] == bs.max_inner_steps(N, k, n_outer, n_inner)
    So = hc.host(ctx.gbm_paths(n_outer, N, 100.0, R, SIG, T, 42, 2))
    want = cv.never_exercising(So, K, R, SIG, T, is_put, k)
    dq = float(np.max(np.abs(d["q"] - want["q"]))) / K
    ds = float(np.max(np.abs(d["samples"] - want["samples"]))) / K
    print(f"never-exercising N={N} k={k}: q deviates {dq:.3e} K, samples {ds:.3e} K")
    assert dq <= CV_TOL and ds <= CV_TOL_WALK
    assert abs(d["q"][0, 0] - E0) <= CV_TOL * K  # every outer path starts at S0
    if k >= N:
        # every sample is Z_N - (Z_N - Q^_0) = E0 up to the walk's rounding, and se_upper is 0.0 up to what E[m^2] - mean^2
        # loses to cancellation: a few roundings of E0^2 (2^-53 relative each) under sqrt(. / pairs)
        print(f"never-exercising N={N} k={k}: upper deviates {abs(d['upper'] - E0) / K:.3e} K")
        assert abs(d["upper"] - E0) <= CV_TOL_WALK * K
        assert d["se_upper"] <= E0 * float(np.sqrt(8 * 2.0 ** -53 / (n_outer // 2)))


# ---------------------------------------------------------------------------------------------- 4. the restatement
_spots = {}


def _case_spots(ctx, p, k, n_lower, n_outer, n_inner):
    """the device's own spots of a case, computed once: they depend on the law and the sizes, not on payoff or policy"""
    key = (int(p.n_steps), k, n_lower, n_outer, n_inner, float(p.S0))
    if key not in _spots:
        _spots[key] = bs.device_spots(ctx, p, k, n_lower, n_outer, n_inner)
    return _spots[key]


RESTATED = [(8, 0, 64, 64, "textbook", True), (8, 0, 64, 64, "given", False), (8, 3, 66, 16, "two_pass", True),
            (7, 0, 16, 192, "reference", True), (7, 6, 16, 192, "given", False), (13, 0, 16, 24, "textbook", True),
            (12, 3, 16, 66, "given", True), (13, 16, 16, 2, "textbook", True), (12, 0, 16, 2, "given", False),
            (7, 3, 16, 24, "given", True), (12, 11, 16, 16, "textbook", True)]


@pytest.mark.parametrize("N,k,n_outer,n_inner,policy,is_put", RESTATED,
                         ids=[f"N{c[0]}-k{c[1]}-o{c[2]}-i{c[3]}-{c[4]}-{'put' if c[5] else 'call'}" for c in RESTATED])
def test_device_equals_restatement(ctx, N, k, n_outer, n_inner, policy, is_put):
    n_lower = 4096
    p = _params(is_put=is_put, N=N)
    given = _given(ctx, p) if policy == "given" else None
    d = ctx.price_american_bounds(p, policy=policy, n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, betas=given,
                                  exercise_every=k, control_variate=True, want_q=True, want_samples=True)
    sp = _case_spots(ctx, p, k, n_lower, n_outer, n_inner)
    dv = cv.check_against_restatement(p, d, sp, k, n_lower, n_outer, n_inner, CV_TOL)
    print(f"restated N={N} k={k} i={n_inner} {policy}: " + ", ".join(f"{key} {v:.3e}" for key, v in dv.items()))
    if k < N and (is_put or policy == "given"):
        assert 0 < d["n_exercised_lower"] < n_lower  # the controlled terms are not all zero


# ---------------------------------------------------------------------------------------------- 5. the lane groups
def test_group_widths_on_the_same_first_pairs(ctx):
    """n_inner = 16 and 32 land in G = 8 and 16; forced to one item per wave (form 1: G = 64) they use the same pairs, so the
    same Q^ up to the order of the sums.  The pairs of an item sit at (i (N+1) + t) n_inner / 2 + j, so the first pairs of a
    call with another n_inner are other pairs: the same item is compared through the restatement of either call."""
    N, n_outer, n_lower = 8, 16, 4096
    p = _params(N=N)
    given = _given(ctx, p)
    try:
        for n_inner in (16, 32, 64, 128):
            kw = dict(policy="given", betas=given, n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, control_variate=True,
                      want_q=True, want_samples=True)
            sp = _case_spots(ctx, p, 0, n_lower, n_outer, n_inner)
            ctx.set_option("bounds_cv_form", 0)
            grouped = ctx.price_american_bounds(p, **kw)
            dvs = [cv.check_against_restatement(p, grouped, sp, 0, n_lower, n_outer, n_inner, CV_TOL)]
            _same_bits(ctx.price_american_bounds(p, **kw), grouped)
            for form in (1,):  # one item per wave
                ctx.set_option("bounds_cv_form", form)
                other = ctx.price_american_bounds(p, **kw)
                dvs.append(cv.check_against_restatement(p, other, sp, 0, n_lower, n_outer, n_inner, CV_TOL))
                assert other["inner_path_steps"] == grouped["inner_path_steps"]
                np.testing.assert_allclose(other["q"], grouped["q"], rtol=0, atol=2 * CV_TOL * K)
                _same_bits(ctx.price_american_bounds(p, **kw), other)
            print(f"restated groups i={n_inner}: " + ", ".join(f"{key} {max(d[key] for d in dvs):.3e}" for key in dvs[0]))
    finally:
        ctx.set_option("bounds_cv_form", 0)


# ---------------------------------------------------------------------------------------------- 6. the statistics
STAT = dict(n_lower=400_000, n_outer=2048)


def test_statistics_at_fifty_dates(ctx):
    p = _params(N=50, M=100_000)
    plain = ctx.price_american_bounds(p, policy="textbook", n_inner=64, **STAT)
    on = ctx.price_american_bounds(p, policy="textbook", n_inner=64, control_variate=True, **STAT)
    plain16 = ctx.price_american_bounds(p, policy="textbook", n_inner=16, **STAT)
    on16 = ctx.price_american_bounds(p, policy="textbook", n_inner=16, control_variate=True, **STAT)
    V = br.lattice(100.0, K, R, SIG, T, 50)
    for name, d in (("plain 64", plain), ("controlled 64", on), ("plain 16", plain16), ("controlled 16", on16)):
        print(f"{name}: [{d['lower']:.5f}, {d['upper']:.5f}] se {d['se_lower']:.5f} / {d['se_upper']:.5f}  lattice {V:.5f}")
    assert abs(on["lower"] - plain["lower"]) <= 4 * float(np.hypot(on["se_lower"], plain["se_lower"]))
    assert on["se_lower"] < plain["se_lower"]
    for d in (on, on16):
        assert d["upper"] >= d["lower"] - 3 * float(np.hypot(d["se_lower"], d["se_upper"]))
        assert d["ci_lo"] <= V <= d["ci_hi"], (d, V)
    assert on16["upper"] < plain16["upper"] - 4 * float(np.hypot(on16["se_upper"], plain16["se_upper"]))


def test_scheduled_game_brackets_its_lattice(ctx):
    """k | N: the scheduled game on the fine paths has the law of the N / k-date game"""
    d = ctx.price_american_bounds(_params(N=48, M=100_000), policy="textbook", n_inner=64, exercise_every=4,
                                  control_variate=True, **STAT)
    V = br.lattice(100.0, K, R, SIG, T, 12)
    print(f"N=48 k=4 controlled: [{d['lower']:.5f}, {d['upper']:.5f}] se {d['se_lower']:.5f} / {d['se_upper']:.5f}  lattice {V:.5f}")
    assert d["ci_lo"] <= V <= d["ci_hi"], (d, V)
    assert d["upper"] >= d["lower"] - 3 * float(np.hypot(d["se_lower"], d["se_upper"]))


# ---------------------------------------------------------------------------------------------- 7. refusals
def _cfg(regressors=0, policy=1):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, 1000, 64, 64
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    return cfg


def _unsupported(ctx):
    """name -> (raw call -> (rc, bytes of the output struct), facade call -> result dict) of the calls with no control variate"""
    lib, h = ctx.lib, ctx.handle
    ph = hc.make_params(hc.HP, scheme=0, is_put=True, S0=100.0, K=K, r=R, T=T, N=8, M=4096, seed=42, stream=0)
    pg = _params()
    pc = _params(is_put=False)

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
    }


def test_refusals_and_the_way_back(ctx):
    calls = _unsupported(ctx)
    before = {name: facade() for name, (_, facade) in calls.items()}
    pd = _params(N=7)
    fresh = _ffi.Context(0)
    try:
        default = fresh.price_american_bounds(pd, control_variate=None, want_q=True, want_samples=True, **TINY)
    finally:
        fresh.close()
    try:
        ctx.set_option("bounds_control_variate", 1)
        for name, (raw, facade) in calls.items():
            rc, out = raw()
            assert rc == -39 and out == b"\xab" * len(out), name  # refused, the output struct untouched
            assert b"bounds_control_variate" in ctx.lib.omc_last_error()
            with pytest.raises(ValueError, match="control"):
                facade()
        # their own argument checks come first: an odd n_inner is still -3
        cfg = _cfg()
        cfg.n_inner = 63
        out = _ffi.BasketBounds()
        pg = _params()
        assert ctx.lib.omc_price_american_basket_bounds(ctx.handle, C.byref(pg), C.byref(cat.basket3()), C.byref(cfg), None,
                                                        None, None, None, C.byref(out)) == -3
        # ... and -38 comes before -39
        ctx.set_option("bounds_exercise_every", 2)
        assert calls["basket"][0]()[0] == -38 and calls["heston spot"][0]()[0] == -39
        ctx.set_option("bounds_exercise_every", 0)
        # an entry point that computes no bounds ignores the option
        assert ctx.price_american(_params(N=7))["price"] > 0
    finally:
        ctx.set_option("bounds_exercise_every", 0)
        ctx.set_option("bounds_control_variate", 0)
    for name, (raw, facade) in calls.items():
        assert raw()[0] == 0, name
        after = facade()
        assert not cat.diff(cat.flat(after), cat.flat(before[name])), name
    # a default call after a controlled one, against a context that never saw the option
    ctx.price_american_bounds(pd, control_variate=True, want_q=True, want_samples=True, **TINY)
    _same_bits(ctx.price_american_bounds(pd, want_q=True, want_samples=True, **TINY), default)
    assert ctx._bounds_cv == 0


# ---------------------------------------------------------------------------------------------- 8. two launches, the fallback
def test_launch_blocks_restated_on_sampled_outer_paths(ctx):
    """At N = 50, n_inner = 512 the worst case is 652,800 steps per outer path: blocks of 1644, two launches for 2048.  Q^ of
    the first, last and a middle outer path of either block and of two partner columns against the restatement."""
    N, n_outer, n_inner = 50, 2048, 512
    per_outer = n_inner * N * (N + 1) // 2
    blk = (1 << 30) // per_outer
    starts = list(range(0, n_outer, blk))
    assert per_outer == 652_800 and blk == 1644 and len(starts) == 2  # a changed launch rule must not empty this test
    rows = []
    for i0 in starts:
        i1 = min(i0 + blk, n_outer)
        rows += [i0, (i0 + i1) // 2, i1 - 1]
    rows += [n_outer // 2 - 1, n_outer // 2]
    assert len(set(rows)) == len(rows) and 0 <= min(rows) and max(rows) < n_outer
    p = _params(N=N, M=20_000)
    d = ctx.price_american_bounds(p, policy="textbook", n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True,
                                  want_samples=True, control_variate=True)
    So = hc.host(ctx.gbm_paths(n_outer, N, 100.0, R, SIG, T, 42, 2))
    inner = br.inner_by_item(lambda off, n: hc.host(ctx.gbm_normals(n, N, 42, 3, off)), So, n_inner,
                             lambda z, s0: hc.host(ctx.gbm_paths_from_normals(z, s0, R, SIG, T)))
    qr = cv.q_rows(So, inner, rows, K, R, SIG, T, True, d["betas"])
    wk = bs.walk_rows(So, qr["q"], rows, K, R, T, True, d["betas"], 0)
    assert qr["ties"] == 0 and wk["ties"] == 0  # numpy's decisions are the device's
    dq = float(np.max(np.abs(d["q"][rows] - qr["q"]))) / K
    ds = float(np.max(np.abs(d["samples"][rows] - wk["samples"]))) / K
    print(f"blocks of {blk}: rows {rows}, q deviates {dq:.3e} K, samples {ds:.3e} K")
    assert dq <= CV_TOL and ds <= CV_TOL_WALK


@pytest.mark.parametrize("k", [0, 3])
def test_deterministic_and_table_fallback(ctx, k):
    p = _params(N=13, M=20_000)
    kw = dict(n_lower=100_000, n_outer=1024, n_inner=24, want_q=True, want_samples=True, exercise_every=k, control_variate=True)
    a = ctx.price_american_bounds(p, **kw)
    b = ctx.price_american_bounds(p, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # every other date decided by the float64 rule: the same decisions
    try:
        c = ctx.price_american_bounds(p, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(b, a)
    _same_bits(c, a)
    assert 0 < a["n_exercised_lower"] < kw["n_lower"]


# ---------------------------------------------------------------------------------------------- 9. the example
def test_c_example_prints_both_brackets(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_bounds_cv"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_bounds_cv.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    N = 12
    out = subprocess.run([str(exe), str(N), "100000", "1024", "128", "16"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    got = {m[0]: (int(m[1]), int(m[2]), float(m[3]), float(m[4]), int(m[5])) for m in re.findall(
        r"(\w+) put, control_variate (\d), n_inner (\d+): bounds \[([-0-9.]+), ([-0-9.]+)\].*inner path-steps (\d+)", out)}
    assert set(got) == {"plain", "controlled"}, out
    for name, on, n_inner in (("plain", False, 128), ("controlled", True, 16)):
        ref = ctx.price_american_bounds(_params(N=N, M=100_000), n_lower=100_000, n_outer=1024, n_inner=n_inner,
                                        control_variate=on)
        v, ni, lo, up, steps = got[name]
        assert (v, ni, steps) == (int(on), n_inner, ref["inner_path_steps"]), (name, out)
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)

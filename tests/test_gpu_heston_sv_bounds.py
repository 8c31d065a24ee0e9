"""Andersen-Broadie price bounds under Heston with a policy on the spot and the variance state
(omc_price_american_bounds_heston with cfg.regressors = 1; options_model_amd/csrc/omc_heston_sv_bounds.hip,
omc_bounds2_dev.h).

The device's Q^_t, samples, bounds and counts against the numpy restatement of tests/helpers/heston_sv_ref.py on the
device's own (spot, variance) states (tests/test_gpu_heston_sv_bounds_fuzz.py runs the same comparison over random shapes);
a call of three inner launches restated on sampled outer paths; the fit, date by date, on the device's own fitting paths;
known answers -- xi = 0 (the variance regressor is truncated away exactly, and the law is GBM), a table without variance
terms (the spot-only call's bits), the selector's default --; what the regressor buys where Feller is violated;
determinism, refusals, the facade and the C example."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_ref as br
from helpers import heston_bounds_case as hc
from helpers import heston_sv_ref as sv
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, T = 100.0, 0.05, 1.0
SEED = 42
FELLER_OFF = dict(v0=0.04, kappa=1.0, theta=0.09, xi=0.9, rho=-0.7)  # 2 kappa theta = 0.18 < xi^2 = 0.81
SETS = dict(feller=hc.HP, off=FELLER_OFF)
REG = sv.REG
BITS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_exercised_lower", "inner_path_steps")


def _params(hp=hc.HP, scheme=0, is_put=True, S0=100.0, N=8, M=4096, stream=0):
    return hc.make_params(hp, scheme=scheme, is_put=is_put, S0=S0, K=K, r=R, T=T, N=N, M=M, seed=SEED, stream=stream)


def _same_bits(a, b, betas=True):
    for k in BITS:
        assert a[k] == b[k], k
    np.testing.assert_array_equal(a["q"], b["q"])
    np.testing.assert_array_equal(a["samples"], b["samples"])
    if betas:
        np.testing.assert_array_equal(a["betas"], b["betas"])


# ---------------------------------------------------------------------------------------------- 1. the restatement
_states = {}


def _case_states(ctx, p, n_lower, n_outer, n_inner, pname):
    """the device's own states of a case, computed once: they depend on the law and the sizes, not on payoff or policy"""
    key = (pname, int(p.heston_scheme), int(p.n_steps), n_lower, n_outer, n_inner)
    if key not in _states:
        _states[key] = sv.device_states(ctx, p, n_lower, n_outer, n_inner, cache=True)
    return _states[key]


TINY = [("textbook", True, 0, "feller"), ("given", False, 0, "feller"), ("textbook", False, 1, "feller"),
        ("given", True, 1, "feller"), ("textbook", True, 1, "off"), ("given", True, 1, "off"), ("textbook", True, 0, "off")]


@pytest.mark.parametrize("policy,is_put,scheme,pname", TINY,
                         ids=[f"{a}-{'put' if b else 'call'}-s{c}-{d}" for a, b, c, d in TINY])
def test_device_equals_restatement(ctx, policy, is_put, scheme, pname):
    N, n_outer, n_inner, n_lower = 8, 32, 64, 4096
    p = _params(SETS[pname], scheme=scheme, is_put=is_put, N=N, M=4096)
    given = sv.given_table(ctx, p) if policy == "given" else None
    d = ctx.price_american_bounds_heston(p, policy=policy, n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, betas=given,
                                         want_q=True, want_samples=True, regressors=REG)
    assert d["betas"].shape == (N + 1, 8)
    if policy == "given":
        np.testing.assert_array_equal(d["betas"], given)
    else:  # the fit, date by date, on the device's own fitting paths
        worst = sv.check_fit(*sv.fitting_paths(ctx, p), K, R, T, is_put, d["betas"], sv.vbar_of(p))
        print(f"fit: largest difference of continuation values {worst:.3g} K")
    assert d["betas"][1:N, 3:6].any()  # the variance is in the rule
    st = _case_states(ctx, p, n_lower, n_outer, n_inner, pname)
    if (scheme, pname) == (1, "off"):  # the lower, outer and inner paths carry negative variance states
        neg = int(np.count_nonzero(st["Yo"][:N] < 0.0))
        print(f"{neg} of {n_outer * N} items start at a negative variance")
        assert st["Yl"].min() < 0.0 and neg > n_outer * N // 20
    if scheme == 0:
        assert st["Yo"].min() >= 0.0
    sv.check_against_restatement(p, d, st, n_lower, n_outer, n_inner)


@pytest.mark.parametrize("scheme", [0, 1])
def test_odd_dates_and_refill_equal_restatement(ctx, scheme):
    """N = 7: the last Philox block is half used and the second draw has three of its four steps; 96 inner pairs for a
    wave's 64 lanes: the finished lanes take the item's next pairs"""
    N, n_outer, n_inner, n_lower = 7, 16, 192, 1000
    p = _params(scheme=scheme, N=N, M=4096)
    d = ctx.price_american_bounds_heston(p, policy="textbook", n_lower=n_lower, n_outer=n_outer, n_inner=n_inner,
                                         want_q=True, want_samples=True, regressors=REG)
    sv.check_against_restatement(p, d, _case_states(ctx, p, n_lower, n_outer, n_inner, "feller"), n_lower, n_outer, n_inner)


def test_generator_starts_at_a_negative_full_truncation_state(ctx):
    """omc_heston_paths_sv_f32 takes a negative v0 with scheme 1, what the inner items above start from: its spots are
    omc_heston_paths_from_normals_f32's from that state bit for bit, row 0 of V is the state, and the first step is the
    deterministic one of a floored variance -- V_1 = fma(kappa dt, theta, v0) for both partners.  Schemes 0 and 2 keep
    refusing it."""
    N, n, stream, off = 13, 200, 7, 11
    hp = FELLER_OFF
    s0, v0 = 93.5, float(np.float32(-0.0123))
    p = _params(hp, scheme=1, N=N)
    S, V = sv.paths_sv(ctx, p, n, stream, off, s0, v0)
    Z = hc.host(ctx.gbm_normals(n // 2, 2 * N, SEED, stream, off))
    X = hc.host(ctx.heston_paths_from_normals(np.ascontiguousarray(Z[0::2]), np.ascontiguousarray(Z[1::2]), s0, R, T, v0,
                                              hp["kappa"], hp["theta"], hp["xi"], hp["rho"], 1))
    np.testing.assert_array_equal(S.view(np.uint32), X.view(np.uint32))
    assert np.all(V[0] == np.float32(v0))
    c = sv.heston_consts(R, T, N, hp["kappa"], hp["theta"], hp["xi"], hp["rho"])
    v1 = np.float32(float(c["kdt"]) * float(c["theta"]) + v0)  # the product is exact in float64
    assert np.all(V[1] == v1) and np.all(S[1] == S[1, 0])
    assert len(np.unique(V[N])) > n // 2  # (V_1 is still negative here: the second step is deterministic too)
    buf = ctx.empty((N + 1, n), np.float32)
    try:
        for scheme in (0, 2):
            assert ctx.lib.omc_heston_paths_sv_f32(ctx.handle, buf.ptr, buf.ptr, n, n, N, s0, R, T, v0, hp["kappa"], hp["theta"],
                                                   hp["xi"], hp["rho"], SEED, stream, off, scheme) == -5
        assert ctx.lib.omc_heston_paths_sv_f32(ctx.handle, buf.ptr, buf.ptr, n, n, N, s0, R, T, float("nan"), hp["kappa"],
                                               hp["theta"], hp["xi"], hp["rho"], SEED, stream, off, 1) == -5
    finally:
        buf.free()


# ---------------------------------------------------------------------------------------------- 2. launch blocks
def test_launch_blocks_restated_on_sampled_outer_paths(ctx):
    """tests/test_gpu_heston_bounds.py's case of three inner launches (N = 50, n_inner = 512: blocks of 822 outer paths for
    2048; no smaller shape splits a call): Q^ of the first, last and a middle outer path of every block, and of the
    antithetic partner columns of two of them, all 50 dates each, against the restatement on the device's own states: q at
    rtol 1e-12, the samples at bounds_ref.samples_atol."""
    N, n_outer, n_inner = 50, 2048, 512
    blk = (1 << 29) // (n_inner // 2 * N * (N + 1))
    starts = list(range(0, n_outer, blk))
    assert blk == 822 and len(starts) == 3  # a changed launch rule must not empty this test
    rows = []
    for i0 in starts:
        i1 = min(i0 + blk, n_outer)
        rows += [i0, (i0 + i1) // 2, i1 - 1]
    rows += [rows[1] + n_outer // 2, rows[2] + n_outer // 2]  # partner columns: other blocks' interiors
    assert len(set(rows)) == len(rows) and max(rows) < n_outer
    p = _params(N=N, M=20_000)
    d = ctx.price_american_bounds_heston(p, policy="textbook", n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True,
                                         want_samples=True, regressors=REG)
    st = sv.device_states(ctx, p, 2, n_outer, n_inner)
    vb = sv.vbar_of(p)
    qr = sv.q_rows(N, st["inner"], rows, K, R, T, True, d["betas"], vb)
    wk = sv.walk_rows(st["Xo"], st["Yo"], qr["q"], rows, K, R, T, True, d["betas"], vb)
    print(f"blocks of {blk}: rows {rows}, ties {qr['ties']} + {wk['ties']}")
    assert qr["ties"] == 0 and wk["ties"] == 0  # numpy's decisions are the device's
    np.testing.assert_allclose(d["q"][rows], qr["q"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d["samples"][rows], wk["samples"], rtol=0, atol=br.samples_atol(N, qr["q"], wk["zmax"]))


# ---------------------------------------------------------------------------------------------- 3. the fit
def _fit_only(ctx, p):
    return ctx.price_american_bounds_heston(p, policy="textbook", n_lower=2, n_outer=2, n_inner=2, regressors=REG)["betas"]


@pytest.mark.parametrize("scheme,pname,is_put,M", [(0, "feller", True, 20_000), (1, "off", True, 20_000),
                                                   (1, "feller", False, 1000), (0, "off", False, 4098)])
def test_fit_date_by_date(ctx, scheme, pname, is_put, M):
    """N = 13 (an odd number of dates), path counts that fill no workgroup evenly and more than one workgroup"""
    p = _params(SETS[pname], scheme=scheme, is_put=is_put, N=13, M=M)
    b = _fit_only(ctx, p)
    X, Y = sv.fitting_paths(ctx, p)
    worst = sv.check_fit(X, Y, K, R, T, is_put, b, sv.vbar_of(p))
    print(f"largest difference of continuation values {worst:.3g} K; n_t {b[1:13, 6]}")
    assert b[1:13, 6].min() > 6 and b[1:13, 3:6].all()
    if (scheme, pname) == (1, "off"):
        assert Y.min() < 0.0


def test_fit_with_a_date_where_nobody_is_in_the_money(ctx):
    """a call from S0 = 70: nobody is above the strike on the first dates; those rows are zeros and nobody exercises there"""
    p = _params(is_put=False, S0=70.0, N=8, M=4096)
    b = _fit_only(ctx, p)
    X, Y = sv.fitting_paths(ctx, p)
    sv.check_fit(X, Y, K, R, T, False, b, sv.vbar_of(p))
    n = b[1:8, 6]
    print("n_t", n)
    assert (n == 0).any() and (n > 6).any() and not b[1:8][n == 0].any()


def test_fit_with_fewer_rows_than_coefficients(ctx):
    """32 paths of a call from S0 = 90: dates with 1 .. 5 paths in the money keep n - 1 features (n < j + 1.5)"""
    p = _params(is_put=False, S0=90.0, N=8, M=32)
    b = _fit_only(ctx, p)
    X, Y = sv.fitting_paths(ctx, p)
    sv.check_fit(X, Y, K, R, T, False, b, sv.vbar_of(p))
    n = b[1:8, 6]
    print("n_t", n)
    few = [t for t in range(1, 8) if 0 < b[t, 6] < 6]
    assert few
    for t in few:
        kept = int(b[t, 6]) - 1
        assert not b[t, 1 + kept:6].any(), (t, b[t])


# ---------------------------------------------------------------------------------------------- 4. known answers
FLAT = dict(v0=0.0625, kappa=2.0, theta=0.0625, xi=0.0, rho=-0.7)  # 0.0625 is exact in float32


def test_zero_vol_of_vol_truncates_the_variance_exactly(ctx):
    """xi = 0 and v0 = theta = 0.0625: the variance stays exactly 0.0625 = vbar, so w = fma(0.0625, 16, -1) = 0 on every
    path, the centred w column is zero and the pivot rule leaves c3 = c4 = c5 = 0 exactly on every date"""
    for scheme in (0, 1):
        p = _params(FLAT, scheme=scheme, N=13, M=4096)
        X, Y = sv.fitting_paths(ctx, p)
        assert np.all(Y == np.float32(0.0625))
        b = _fit_only(ctx, p)
        assert b[1:13, 6].min() > 100 and b[1:13, :3].all() and not b[:, 3:6].any()
        sv.check_fit(X, Y, K, R, T, True, b, 0.0625)


@pytest.mark.parametrize("S0", [90.0, 100.0, 110.0])
def test_zero_vol_of_vol_brackets_the_gbm_lattice(ctx, S0):
    """... and the law is GBM at sigma = 0.25: the bracket contains the lattice value and is as tight as
    tests/test_gpu_heston_bounds.py asks of the spot-only call there (its threshold and its sizes: the gap is a bias and
    noise statement that the tiny shapes of this file do not resolve)"""
    N = 50
    d = ctx.price_american_bounds_heston(_params(FLAT, S0=S0, N=N, M=100_000), policy="textbook", n_lower=400_000,
                                         n_outer=4096, n_inner=512, regressors=REG)
    assert not d["betas"][:, 3:6].any()
    V = br.lattice(S0, K, R, 0.25, T, N)
    print(S0, d["lower"], d["se_lower"], d["upper"], d["se_upper"], V)
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)
    assert 0.0 < d["upper"] - d["lower"] < 0.02 * V, (d, V)


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("is_put", [True, False])
def test_table_without_variance_terms_gives_the_spot_calls_bits(ctx, scheme, is_put):
    """c3 = c4 = c5 = 0: every output of the two-regressor kernels has the bits of the spot-only call given (c0, c1, c2, n)
    -- the decisions of the float64 rule are those of the exercise tables, and the sums are formed alike.  The Feller-violating
    set: negative variance states go through the polynomial with coefficient 0."""
    p = _params(FELLER_OFF, scheme=scheme, is_put=is_put, N=13, M=4096)
    kw = dict(n_lower=4096, n_outer=64, n_inner=192, want_q=True, want_samples=True)
    b4 = ctx.price_american_bounds_heston(p, policy="textbook", **kw)["betas"]
    assert b4[1:13, 3].min() > 6
    a = ctx.price_american_bounds_heston(p, policy="given", betas=b4, **kw)
    b = ctx.price_american_bounds_heston(p, policy="given", betas=sv.lifted_table(b4), regressors=REG, **kw)
    _same_bits(a, b, betas=False)
    np.testing.assert_array_equal(sv.spot_table(b["betas"]), a["betas"])
    assert 0 < a["n_exercised_lower"] < 4096


def test_selector_zero_is_the_spot_call(ctx):
    """regressors "spot" / 0 through the new field: the bits of a call that leaves the field alone"""
    p = _params(N=13, M=4096)
    kw = dict(n_lower=4096, n_outer=64, n_inner=192, want_q=True, want_samples=True)
    a = ctx.price_american_bounds_heston(p, **kw)
    assert a["betas"].shape == (14, 4)
    for reg in ("spot", 0):
        _same_bits(a, ctx.price_american_bounds_heston(p, regressors=reg, **kw))


# ---------------------------------------------------------------------------------------------- 5. what the regressor buys
def test_variance_regressor_raises_the_lower_bound_where_feller_is_violated(ctx):
    """v0 = 0.04, theta = 0.09, kappa = 1, xi = 0.9, rho = -0.7, ATM put, N = 10, full truncation; both policies fitted on
    the same 100,000 paths and applied to the same streams.  A float64 numpy restatement (400,000 fresh paths) puts the
    paired difference of the lower bounds at +0.207 (se 0.009), 9 times the combined standard error of the two unpaired
    estimates: the restatement clears the asserted 3 units three times over.  The spot-only upper bound holds against
    policies that see the variance, so the new lower bound must stay below it.  How far the upper bound moves has no
    threshold: it is printed."""
    p = _params(FELLER_OFF, scheme=1, N=10, M=100_000)
    kw = dict(policy="textbook", n_lower=400_000, n_outer=2048, n_inner=256)
    spot = ctx.price_american_bounds_heston(p, **kw)
    both = ctx.price_american_bounds_heston(p, regressors=REG, **kw)
    se = math.hypot(both["se_lower"], spot["se_lower"])
    gain = both["lower"] - spot["lower"]
    print(f"spot          [{spot['lower']:.4f} ({spot['se_lower']:.4f}), {spot['upper']:.4f} ({spot['se_upper']:.4f})]  "
          f"steps {spot['inner_path_steps']}")
    print(f"spot+variance [{both['lower']:.4f} ({both['se_lower']:.4f}), {both['upper']:.4f} ({both['se_upper']:.4f})]  "
          f"steps {both['inner_path_steps']}")
    print(f"lower bound +{gain:.4f} = {gain / se:.1f} combined standard errors; upper bound {both['upper'] - spot['upper']:+.4f}; "
          f"gap {spot['upper'] - spot['lower']:.4f} -> {both['upper'] - both['lower']:.4f}")
    assert gain > 3 * se, (gain, se)
    assert both["lower"] - 3 * both["se_lower"] <= both["upper"] + 3 * both["se_upper"], both
    assert both["lower"] <= spot["upper"] + 3 * math.hypot(both["se_lower"], spot["se_upper"]), (both, spot)


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_deterministic_and_no_exercise_tables(ctx):
    p = _params(FELLER_OFF, scheme=1, N=13, M=4096)
    kw = dict(n_lower=4096, n_outer=64, n_inner=192, want_q=True, want_samples=True, regressors=REG)
    a = ctx.price_american_bounds_heston(p, **kw)
    b = ctx.price_american_bounds_heston(p, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # there are no float32 exercise tables: no effect
    try:
        c = ctx.price_american_bounds_heston(p, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(a, b)
    _same_bits(a, c)


# ---------------------------------------------------------------------------------------------- 7. refusals
def _rc(ctx, p, policy=1, regressors=1, n_lower=1000, n_outer=64, n_inner=64, betas=None):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    b = None if betas is None else np.ascontiguousarray(betas, np.float64)
    return ctx.lib.omc_price_american_bounds_heston(ctx.handle, C.byref(p), C.byref(cfg),
                                                    b.ctypes.data if b is not None else None, None, None, None, C.byref(out))


def test_refusals(ctx):
    p = _params()
    assert _rc(ctx, p) == 0
    assert _rc(ctx, p, policy=0) == -4 and _rc(ctx, p, policy=2) == -4  # reference, two_pass
    assert _rc(ctx, p, policy=7) == -4
    assert _rc(ctx, p, regressors=2) == -4 and _rc(ctx, p, regressors=-1) == -4
    assert _rc(ctx, p, policy=0, regressors=0) == 0  # the spot-only call keeps its policies
    assert _rc(ctx, _params(dict(hc.HP, v0=0.0, theta=0.0))) == -5
    assert _rc(ctx, _params(dict(hc.HP, v0=0.0, theta=-0.01))) == -5
    assert _rc(ctx, _params(N=513), n_outer=2, n_inner=2) == -16
    assert _rc(ctx, _params(N=512, M=64), n_lower=2, n_outer=2, n_inner=2) == 0
    assert _rc(ctx, _params(scheme=2)) == -12
    assert _rc(ctx, p, policy=3) == -7  # given without a table
    assert _rc(ctx, p, n_inner=63) == -3 and _rc(ctx, p, n_outer=63) == -3 and _rc(ctx, p, n_lower=999) == -3
    assert _rc(ctx, _params(N=252), n_outer=1 << 14, n_inner=1 << 12) == -16
    out = _ffi.Bounds()
    assert ctx.lib.omc_price_american_bounds_heston(ctx.handle, C.byref(p), None, None, None, None, None, C.byref(out)) == -7
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _rc(hooked, p) == -10
    finally:
        hooked.close()


# ---------------------------------------------------------------------------------------------- 8. interfaces
def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_bounds_heston

    kw = dict(n_lower=4096, n_outer=64, n_inner=192)
    f = price_american_bounds_heston(100.0, K, R, T, 4096, 13, FELLER_OFF, heston_scheme="full_truncation", seed=SEED,
                                     stream=5, ctx=ctx, regressors=REG, **kw)
    d = ctx.price_american_bounds_heston(_params(FELLER_OFF, scheme=1, N=13, M=4096, stream=5), regressors=REG, **kw)
    assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                              d["se_upper"], d["inner_path_steps"])
    np.testing.assert_array_equal(f.betas, d["betas"])
    assert f.betas.shape == (14, 8) and f.regressors == REG and f.variance_scale == 0.09 and f.policy == "textbook"
    g = price_american_bounds_heston(100.0, K, R, T, 4096, 13, FELLER_OFF, heston_scheme="full_truncation", seed=SEED,
                                     stream=5, ctx=ctx, policy="given", betas=f.betas, regressors=REG, **kw)
    assert (g.lower, g.upper) == (f.lower, f.upper)
    s = price_american_bounds_heston(100.0, K, R, T, 4096, 13, FELLER_OFF, heston_scheme="full_truncation", seed=SEED,
                                     stream=5, ctx=ctx, **kw)
    assert s.regressors == "spot" and s.betas.shape == (14, 4) and s.variance_scale == 0.09


def test_c_example_prints_both_brackets(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_heston_sv_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_heston_sv_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "13", "4096", "64", "192", "1"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    got = re.findall(r"policy on (\S+), 13 dates: bounds \[([-0-9.]+), ([-0-9.]+)\]", out)
    assert [g[0] for g in got] == ["spot", "spot+variance"], out
    p = _params(scheme=1, N=13, M=100_000)
    for (_, lo, up), reg in zip(got, ("spot", REG)):
        ref = ctx.price_american_bounds_heston(p, n_lower=4096, n_outer=64, n_inner=192, regressors=reg)
        assert abs(float(lo) - ref["lower"]) < 1e-6 and abs(float(up) - ref["upper"]) < 1e-6, (out, ref)
    assert len(re.findall(r"inner path-steps \d+", out)) == 2 and out.count("kernels:") == 2

"""Andersen-Broadie price bounds under Heston (omc_price_american_bounds_heston, omc_heston_paths_sv_f32;
options_model_amd/csrc/omc_heston_bounds.hip).

The generator that keeps the variance against omc_heston_paths_f32 (bits) and against a restart from its own state; the
device's Q^_t, samples, bounds and counts against the numpy restatement of tests/helpers/bounds_ref.py on the device's own
spots (tests/helpers/heston_bounds_case.py; tests/test_gpu_heston_bounds_fuzz.py runs the same comparison over random
shapes); a call of three inner launches restated on sampled outer paths; known answers -- one date, xi = 0 (GBM), the call
(European in the discretised model), a never-exercising table, the put against its European --; determinism, refusals,
the facade and the C example."""
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
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, T = 100.0, 0.05, 1.0
SEED = 42  # (no tie of numpy's unfused arithmetic at this seed in any case below)
SETS = dict(feller=hc.HP, clamp=hc.HP_CLAMP)
SCHEMES = {0: "reference", 1: "full_truncation", 2: "calibrator"}


def _params(hp=hc.HP, scheme=0, is_put=True, S0=100.0, N=8, M=4096, stream=0):
    return hc.make_params(hp, scheme=scheme, is_put=is_put, S0=S0, K=K, r=R, T=T, N=N, M=M, seed=SEED, stream=stream)


# ---------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize("scheme", [0, 1, 2])
@pytest.mark.parametrize("M,N", [(4096, 50), (1000, 13), (10, 3), (2, 1)])
def test_sv_generator_keeps_the_spots_bits(ctx, M, N, scheme):
    hp = list(hc.HP.values())
    S = hc.host(ctx.heston_paths(M, N, 100.0, R, T, *hp, SEED, 5, 3, scheme))
    Sd, Vd = ctx.heston_paths_sv(M, N, 100.0, R, T, *hp, SEED, 5, 3, scheme)
    S2, V = hc.host(Sd), hc.host(Vd)
    np.testing.assert_array_equal(S2.view(np.uint32), S.view(np.uint32))
    assert V.shape == S.shape and np.all(V[0] == np.float32(hc.HP["v0"]))
    assert np.all(np.isfinite(V))
    if scheme == 0:
        assert V.min() >= 0.0
    if scheme == 2:
        assert V.min() >= np.float32(1e-8)
    assert np.any(V[1:, :M // 2] != V[1:, M // 2:])  # the partners' variances are their own


@pytest.mark.parametrize("scheme,pname", [(0, "feller"), (1, "feller"), (2, "feller"), (0, "clamp"), (1, "clamp")])
def test_sv_state_restarts_the_path(ctx, scheme, pname):
    """(S[t, j], V[t, j]) is the state after step t: heston_paths_from_normals started there with the generator's
    remaining normals (rows 2(k-1), 2(k-1)+1 of gbm_normals are (z1, z2) of step k) reproduces rows t+1 .. N of that
    column bit for bit -- the first partner in the first output column, the antithetic partner (started at ITS state) in
    the second.  The from-normals entry point takes dt = T / rows, so the remaining N - t rows are padded to N with zeros
    and the rows after N - t dropped.  With the clamp set scheme 1 stores negative variances, and they restart too."""
    M, N, stream, off = 1000, 13, 5, 7
    P = M // 2
    hp = SETS[pname]
    h = list(hp.values())
    Sd, Vd = ctx.heston_paths_sv(M, N, 100.0, R, T, *h, SEED, stream, off, scheme)
    S, V = hc.host(Sd), hc.host(Vd)
    Z = hc.host(ctx.gbm_normals(P, 2 * N, SEED, stream, off))
    z1, z2 = Z[0::2], Z[1::2]
    if (scheme, pname) == (1, "clamp"):
        assert V.min() < 0.0  # Feller is violated: full truncation carries negative variances
    if scheme == 0:
        assert V.min() >= 0.0 and (pname == "feller" or (V == 0.0).any())
    for t in (0, 4, 12):
        low = np.argsort(np.minimum(V[t, :P], V[t, P:]))[:4]  # the pairs with the lowest variance state at t
        for j in sorted({0, 1, 2, P - 1, *[int(x) for x in low]}):
            pad1, pad2 = np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32)
            pad1[:N - t, 0], pad2[:N - t, 0] = z1[t:, j], z2[t:, j]
            for col, out_col in ((j, 0), (j + P, 1)):
                X = hc.host(ctx.heston_paths_from_normals(pad1, pad2, float(S[t, col]), R, T, float(V[t, col]), hp["kappa"],
                                                          hp["theta"], hp["xi"], hp["rho"], scheme))
                np.testing.assert_array_equal(X[1:N - t + 1, out_col].view(np.uint32), S[t + 1:, col].view(np.uint32),
                                              err_msg=f"t {t} column {col}")


# ---------------------------------------------------------------------------------------------- 2. the restatement
_spots = {}


def _case_spots(ctx, p, n_lower, n_outer, n_inner, pname):
    """the device's own spots of a case, computed once: they depend on the law and the sizes, not on payoff or policy"""
    key = (pname, int(p.heston_scheme), int(p.n_steps), n_lower, n_outer, n_inner)
    if key not in _spots:
        _spots[key] = hc.device_spots(ctx, p, n_lower, n_outer, n_inner, cache=True)
    return _spots[key]


TINY = [(pol, put, 0, "feller") for pol in hc.POLICIES for put in (True, False)] + [("textbook", True, 1, "clamp")]


@pytest.mark.parametrize("policy,is_put,scheme,pname", TINY,
                         ids=[f"{a}-{'put' if b else 'call'}-s{c}-{d}" for a, b, c, d in TINY])
def test_device_equals_restatement(ctx, policy, is_put, scheme, pname):
    N, n_outer, n_inner, n_lower = 8, 64, 64, 4096
    p = _params(SETS[pname], scheme=scheme, is_put=is_put, N=N, M=4096)
    given = hc.given_table(ctx, p) if policy == "given" else None
    d = ctx.price_american_bounds_heston(p, policy=policy, n_lower=n_lower, n_outer=n_outer, n_inner=n_inner, betas=given,
                                         want_q=True, want_samples=True)
    if policy == "given":
        np.testing.assert_array_equal(d["betas"], given)
    else:  # omc_lsm_poly's fits on the Heston paths of p
        np.testing.assert_array_equal(d["betas"], hc.fitted_table(ctx, p, policy))
    sp = _case_spots(ctx, p, n_lower, n_outer, n_inner, pname)
    if (scheme, pname) == (1, "clamp"):
        assert sp["Vo"].min() < 0.0  # inner simulations start at negative variance states too
    hc.check_against_restatement(p, d, sp, n_lower, n_outer, n_inner)


@pytest.mark.parametrize("scheme", [0, 1])
def test_odd_dates_and_refill_equal_restatement(ctx, scheme):
    """N = 7: the last Philox block is half used and the second draw has three of its four steps; 96 inner pairs for a
    wave's 64 lanes: the finished lanes take the item's next pairs"""
    N, n_outer, n_inner, n_lower = 7, 16, 192, 1000
    p = _params(scheme=scheme, N=N, M=4096)
    d = ctx.price_american_bounds_heston(p, policy="textbook", n_lower=n_lower, n_outer=n_outer, n_inner=n_inner,
                                         want_q=True, want_samples=True)
    hc.check_against_restatement(p, d, _case_spots(ctx, p, n_lower, n_outer, n_inner, "feller"), n_lower, n_outer, n_inner)


# GPU sizes of a few seconds (those of tests/test_gpu_bounds.py)
BIG = dict(n_lower=400_000, n_outer=4096, n_inner=512)


# ---------------------------------------------------------------------------------------------- 3. launch blocks
def test_launch_blocks_restated_on_sampled_outer_paths(ctx):
    """A Heston step draws two normals, so an inner launch covers at most 2^29 worst-case inner steps (n_inner N (N+1) / 2
    per outer path): at N = 50, n_inner = 512 that is blocks of 822 outer paths, three launches for 2048.  Q^ of the first,
    last and a middle outer path of every block, and of the antithetic partner columns of two of them, all 50 dates each,
    against the restatement on the device's own spots: q at rtol 1e-12, the samples at bounds_ref.samples_atol."""
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
                                         want_samples=True)
    sp = hc.device_spots(ctx, p, 2, n_outer, n_inner)
    qr = br.q_rows(sp["So"], sp["inner"], rows, K, R, T, True, d["betas"])
    wk = br.walk_rows(sp["So"], qr["q"], rows, K, R, T, True, d["betas"])
    print(f"blocks of {blk}: rows {rows}, ties {qr['ties']} + {wk['ties']}")
    assert qr["ties"] == 0 and wk["ties"] == 0  # numpy's decisions are the device's
    np.testing.assert_allclose(d["q"][rows], qr["q"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d["samples"][rows], wk["samples"], rtol=0, atol=br.samples_atol(N, qr["q"], wk["zmax"]))


# ---------------------------------------------------------------------------------------------- 4. known answers
_euro = {}


def _european(ctx, scheme, is_put, N=50):
    """omc_price_european of the same scheme and n_steps at 4M paths -> (price, standard error)"""
    from options_model_amd import price_european_option

    if (scheme, is_put, N) not in _euro:
        e = price_european_option(100.0, K, R, 0.2, T, 4_000_000, N, model="Heston", option_type="put" if is_put else "call",
                                  heston_params=hc.HP, heston_scheme=SCHEMES[scheme], seed=SEED, stream=11, ctx=ctx)
        _euro[(scheme, is_put, N)] = (e.price, e.stderr)
    return _euro[(scheme, is_put, N)]


@pytest.mark.parametrize("is_put", [True, False])
def test_one_date_is_black_scholes(ctx, is_put):
    """one log-Euler step at the fixed variance v0 is exactly lognormal with sigma = sqrt(v0)"""
    d = ctx.price_american_bounds_heston(_params(is_put=is_put, N=1, M=4096), **BIG)
    bs = br.black_scholes(100.0, K, R, math.sqrt(hc.HP["v0"]), T, is_put)
    print(d["lower"], d["se_lower"], d["upper"], d["se_upper"], bs)
    assert abs(d["lower"] - bs) <= 4 * d["se_lower"], (d, bs)
    assert abs(d["upper"] - bs) <= 4 * d["se_upper"], (d, bs)
    assert d["n_exercised_lower"] == 0
    assert d["inner_path_steps"] == BIG["n_outer"] * BIG["n_inner"]


@pytest.mark.parametrize("S0", [90.0, 100.0, 110.0])
def test_zero_vol_of_vol_brackets_the_gbm_lattice(ctx, S0):
    """xi = 0 and v0 = theta: kdt (theta - v) = 0 and xi sqrt(dt) w = 0, so the variance stays exactly theta and the law is
    GBM at sigma = 0.2; the gap threshold is the GBM test's (the same law)"""
    N = 50
    hp = dict(hc.HP, xi=0.0)
    d = ctx.price_american_bounds_heston(_params(hp, S0=S0, N=N, M=100_000), policy="textbook", **BIG)
    V = br.lattice(S0, K, R, 0.2, T, N)
    print(S0, d["lower"], d["se_lower"], d["upper"], d["se_upper"], V)
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)
    assert 0.0 < d["upper"] - d["lower"] < 0.02 * V, (d, V)


@pytest.mark.parametrize("scheme", [0, 1])
def test_call_bracket_contains_the_european(ctx, scheme):
    """E[exp(-r dt) S_{t+1} | S_t, v_t] = S_t for the log-Euler step, so the discounted spot is a martingale and the
    Bermudan call of the discretised model is its European call"""
    d = ctx.price_american_bounds_heston(_params(scheme=scheme, is_put=False, N=50, M=100_000), policy="textbook", **BIG)
    eu, se = _european(ctx, scheme, False)
    print(scheme, d["lower"], d["se_lower"], d["upper"], d["se_upper"], eu, se)
    assert d["lower"] - 3 * d["se_lower"] <= eu + 3 * se, (d, eu, se)
    assert eu - 3 * se <= d["upper"] + 3 * d["se_upper"], (d, eu, se)


def test_never_exercise_table_gives_the_european(ctx):
    N = 50
    d = ctx.price_american_bounds_heston(_params(N=N), policy="given", betas=np.zeros((N + 1, 4)), **BIG)
    eu, se = _european(ctx, 0, True)
    print(d["lower"], d["se_lower"], eu, se)
    assert abs(d["lower"] - eu) <= 4 * math.hypot(d["se_lower"], se), (d, eu, se)
    assert d["n_exercised_lower"] == 0
    assert d["inner_path_steps"] == BIG["n_outer"] * BIG["n_inner"] * N * (N + 1) // 2


@pytest.mark.parametrize("scheme", [0, 1])
def test_put_bracket_is_ordered_and_above_the_european(ctx, scheme):
    """the gap of the spot-only policy has no threshold fixed in advance: tools/time_heston_bounds.py measures it
    """
    d = ctx.price_american_bounds_heston(_params(scheme=scheme, N=50, M=100_000), policy="textbook", **BIG)
    eu, se = _european(ctx, scheme, True)
    print(scheme, d["lower"], d["se_lower"], d["upper"], d["se_upper"], eu, se)
    assert d["upper"] + 3 * d["se_upper"] >= d["lower"] - 3 * d["se_lower"], d
    assert d["lower"] + 3 * d["se_lower"] >= eu - 3 * se, (d, eu, se)


# ---------------------------------------------------------------------------------------------- 5. determinism
def test_deterministic_and_table_fallback(ctx):
    p = _params(N=50, M=20_000)
    kw = dict(n_lower=100_000, n_outer=2048, n_inner=256, want_q=True, want_samples=True)
    a = ctx.price_american_bounds_heston(p, **kw)
    b = ctx.price_american_bounds_heston(p, **kw)
    # every other step decided by the float64 rule instead of the tables: the same decisions, the same bits
    ctx.set_option("pass2_tables_irregular_every", 2)
    try:
        c = ctx.price_american_bounds_heston(p, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    for x in (b, c):
        for k in ("lower", "se_lower", "upper", "se_upper", "n_exercised_lower", "inner_path_steps"):
            assert x[k] == a[k], k
        np.testing.assert_array_equal(x["q"], a["q"])
        np.testing.assert_array_equal(x["samples"], a["samples"])
        np.testing.assert_array_equal(x["betas"], a["betas"])


# ---------------------------------------------------------------------------------------------- 6. refusals
def _rc(ctx, p, policy=1, n_lower=1000, n_outer=64, n_inner=64, betas=None):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    b = None if betas is None else np.ascontiguousarray(betas, np.float64)
    return ctx.lib.omc_price_american_bounds_heston(ctx.handle, C.byref(p), C.byref(cfg),
                                                    b.ctypes.data if b is not None else None, None, None, None, C.byref(out))


def test_refusals(ctx):
    p = _params()
    gbm = _ffi.make_params(model="gbm", is_put=True, semantics="two_pass", n_paths=4096, n_steps=8, S0=100.0, K=K, r=R,
                           sigma=0.2, T=T, seed=SEED)
    assert _rc(ctx, gbm) == -12
    assert _rc(ctx, _params(scheme=2)) == -12  # the calibrator's scheme
    assert _rc(ctx, p, n_inner=63) == -3
    assert _rc(ctx, p, n_outer=63) == -3
    assert _rc(ctx, p, n_lower=999) == -3
    assert _rc(ctx, p, policy=7) == -4
    assert _rc(ctx, p, policy=3) == -7  # given without a table
    assert _rc(ctx, _params(N=252), n_outer=1 << 14, n_inner=1 << 12) == -16
    with pytest.raises(ValueError):
        ctx.price_american_bounds_heston(p, policy="given", betas=np.zeros((5, 4)), n_lower=1000, n_outer=64, n_inner=64)
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _rc(hooked, p) == -10
    finally:
        hooked.close()
    S = ctx.empty((4, 10), np.float32)  # the generator: a null V
    try:
        assert ctx.lib.omc_heston_paths_sv_f32(ctx.handle, S.ptr, None, 10, 10, 3, 100.0, R, T, 0.04, 2.0, 0.04, 0.3, -0.7,
                                               SEED, 0, 0, 0) == -7
        assert ctx.lib.omc_heston_paths_sv_f32(ctx.handle, S.ptr, S.ptr, 10, 9, 3, 100.0, R, T, 0.04, 2.0, 0.04, 0.3, -0.7,
                                               SEED, 0, 0, 0) == -3
    finally:
        S.free()


# ---------------------------------------------------------------------------------------------- 7. interfaces
def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_bounds_heston

    kw = dict(n_lower=100_000, n_outer=1024, n_inner=256)
    f = price_american_bounds_heston(100.0, K, R, T, 20_000, 50, hc.HP, heston_scheme="full_truncation", seed=SEED, stream=5,
                                     ctx=ctx, **kw)
    d = ctx.price_american_bounds_heston(_params(scheme=1, N=50, M=20_000, stream=5), **kw)
    assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                              d["se_upper"], d["inner_path_steps"])
    np.testing.assert_array_equal(f.betas, d["betas"])
    assert f.policy == "textbook" and set(f.timings_ms) == {"fit", "lower", "upper", "total"}
    with pytest.raises(ValueError):
        price_american_bounds_heston(100.0, K, R, T, 20_000, 50, hc.HP, n_inner=255, ctx=ctx)
    with pytest.raises(ValueError):
        price_american_bounds_heston(100.0, K, R, T, 20_000, 50, hc.HP, heston_scheme="calibrator", ctx=ctx)


def test_c_example_prints_the_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_heston_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_heston_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "50", "200000", "2048", "256"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    ref = ctx.price_american_bounds_heston(_params(N=50, M=100_000), n_lower=200_000, n_outer=2048, n_inner=256)
    lo, up = (float(v) for v in re.search(r"bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
    assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
    assert re.search(r"inner path-steps \d+", out) and "kernels:" in out
    assert not math.isnan(lo)

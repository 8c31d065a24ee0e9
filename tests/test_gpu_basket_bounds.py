"""Andersen-Broadie bounds on the index of several correlated GBM assets (omc_price_american_basket_bounds,
options_model_amd/csrc/omc_basket_bounds.hip).

  1. d = 1, w = 1, q = 0               the bits of omc_price_american_bounds: bounds, errors, Q^, samples, policy, counts
  2. d = 2, 3, 8 x the three kinds     the numpy restatement of tests/helpers/bounds_ref.py on the device's own index
                                       spots (helpers/basket_bounds_case.py: lower / outer matrices and one restart call of
                                       omc_price_american_basket per inner item), no ties, equal counts, rtol 1e-12
  3. several inner launches            the 2^30 / d rule at d = 2: three launches, sampled outer paths restated
  4. the bracket                       the two-asset max-call benchmark and a single asset with a yield against their
                                       lattices (helpers/basket_lattice.py) within 3 standard errors
  5. known answers, 6. determinism and the float64 fallback, 7. refusals, 8. the facade and the C example
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import basket_bounds_case as bc
from helpers import basket_lattice as bl
from helpers import bounds_ref as br
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R = 100.0, 0.05
POLICIES = ["textbook", "two_pass", "reference", "given"]
RHO3 = bc.RHO3
_basket = bc.unequal_basket  # unequal spots, sigmas, yields and weights; a non-trivial correlation


def _params(is_put=True, N=8, M=4096, stream=0, model="gbm", T=1.0, S0=100.0, sigma=0.2, seed=42):
    return _ffi.make_params(model=model, is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N, S0=S0, K=K, r=R,
                            sigma=sigma, T=T, seed=seed, stream=stream)


# ------------------------------------------------------------------ 1. one asset: the vanilla entry, bit for bit
def _given_table(ctx, N, is_put):
    """a policy from other paths (stream 9), textbook fits"""
    S = ctx.gbm_paths(4096, N, 100.0, R, 0.2, 1.0, 42, 9)
    d = ctx.lsm_poly(S, K, R, 1.0, is_put, "textbook")
    S.free()
    b = np.zeros((N + 1, 4))
    b[:, :3], b[:, 3] = d["betas"], d["nitm"]
    return b


@pytest.mark.parametrize("n_inner", [64, 200])  # 200: 100 pairs > 64 lanes, the refill
@pytest.mark.parametrize("N", [8, 9])  # 9: a partial Philox block
@pytest.mark.parametrize("policy", POLICIES)
def test_one_asset_is_the_vanilla_entry_bit_for_bit(ctx, policy, N, n_inner):
    for i, is_put in enumerate((True, False)):
        kind = bc.KINDS[(i + N + POLICIES.index(policy)) % 3]
        p = _params(is_put=is_put, N=N)
        given = _given_table(ctx, N, is_put) if policy == "given" else None
        kw = dict(policy=policy, n_lower=4096, n_outer=64, n_inner=n_inner, betas=given, want_q=True, want_samples=True)
        v = ctx.price_american_bounds(p, **kw)
        b = ctx.price_american_basket_bounds(p, _ffi.make_basket([100.0], [0.2], [0.0], [1.0], kind=kind), **kw)
        for k in ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_exercised_lower", "inner_path_steps",
                  "n_lower", "n_outer", "n_inner"):
            assert b[k] == v[k], (k, kind, is_put)
        for k in ("q", "samples", "betas"):
            np.testing.assert_array_equal(b[k], v[k], err_msg=f"{k} {kind} {is_put}")
        assert (b["n_assets"], b["kind"], b["index0"]) == (1, _ffi.BASKET_KINDS[kind], 100.0)
        assert not math.isnan(b["lower"]) and b["inner_path_steps"] > 0


# ------------------------------------------------------------------ 2. several assets: the restatement
@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("d", [2, 3, 8])
def test_device_equals_restatement(ctx, d, kind):
    N, n_outer, n_inner, n_lower = 6, 32, 64, 2048
    j = [2, 3, 8].index(d) * 3 + bc.KINDS.index(kind)
    policy, is_put = POLICIES[j % 4], j % 2 == 0
    p, b = _params(is_put=is_put, N=N), _basket(d, kind)
    given = bc.fuzz_given_table(ctx, p, b, np.zeros(N + 1, bool)) if policy == "given" else None
    dev = ctx.price_american_basket_bounds(p, b, policy=policy, n_lower=n_lower, n_outer=n_outer, n_inner=n_inner,
                                           betas=given, want_q=True, want_samples=True)
    if policy == "given":
        np.testing.assert_array_equal(dev["betas"], given)
    else:  # omc_lsm_poly's fits on the device's own index matrix of p
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, b, policy))
    lo, up = bc.check_against_restatement(ctx, p, b, dev, n_lower, n_outer, n_inner)
    assert up["inner_path_steps"] >= n_outer * n_inner and dev["n_assets"] == d


# ------------------------------------------------------------------ 3. several launches of the inner kernel
def test_launch_blocks_restated_on_sampled_outer_paths(ctx):
    """Each inner launch covers at most 2^30 / d worst-case inner path steps: at d = 2, N = 50,
    n_inner = 512 that is blocks of 822 outer paths, three launches for 2048.  Q^ of the first, last and a middle outer
    path of every block and of the partner columns of two of them against the restatement, with the tolerances of
    tests/test_gpu_bounds.py's launch-block test."""
    d, N, n_outer, n_inner = 2, 50, 2048, 512
    blk = ((1 << 30) // d) // (n_inner // 2 * N * (N + 1))
    starts = list(range(0, n_outer, blk))
    assert blk == 822 and len(starts) == 3  # a changed launch rule must not empty this test
    rows = []
    for i0 in starts:
        i1 = min(i0 + blk, n_outer)
        rows += [i0, (i0 + i1) // 2, i1 - 1]
    rows += [rows[1] + n_outer // 2, rows[2] + n_outer // 2]  # partner columns: other blocks' interiors
    assert len(set(rows)) == len(rows) and max(rows) < n_outer
    p, b = _params(N=N, M=20_000), _basket(d, "best-of")
    dev = ctx.price_american_basket_bounds(p, b, policy="textbook", n_lower=4096, n_outer=n_outer, n_inner=n_inner,
                                           want_q=True, want_samples=True)
    sp = bc.device_spots(ctx, p, b, 2, n_outer, n_inner)
    try:
        qr = br.q_rows(sp["So"], sp["inner"], rows, K, R, 1.0, True, dev["betas"])
    finally:
        sp["free"]()
    wk = br.walk_rows(sp["So"], qr["q"], rows, K, R, 1.0, True, dev["betas"])
    print(f"blocks of {blk}: rows {rows}, ties {qr['ties']} + {wk['ties']}")
    assert qr["ties"] == 0 and wk["ties"] == 0  # numpy's decisions are the device's
    np.testing.assert_allclose(dev["q"][rows], qr["q"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(dev["samples"][rows], wk["samples"], rtol=0, atol=br.samples_atol(N, qr["q"], wk["zmax"]))


# ------------------------------------------------------------------ 4. the bracket
BIG = dict(n_lower=400_000, n_outer=4096, n_inner=512)


@pytest.mark.parametrize("S0", [90.0, 100.0, 110.0])
def test_brackets_the_max_call_benchmark(ctx, S0):
    """Two-asset max-call, nine dates (Broadie-Glasserman / Andersen-Broadie 2004; published 8.075 / 13.902 / 21.345): the
    lattice value lies between the bounds.  The policy sees the index alone, so the bracket is percent-wide (DESIGN.md
    17.5 has the measured ones)."""
    p = _params(is_put=False, N=9, M=100_000, T=3.0, S0=S0)
    b = _ffi.make_basket([S0, S0], [0.2, 0.2], [0.1, 0.1], [1.0, 1.0], None, "best-of")
    d = ctx.price_american_basket_bounds(p, b, policy="textbook", **BIG)
    V = bl.two_asset((S0, S0), K, R, (0.2, 0.2), 3.0, 9, 80, yields=(0.1, 0.1), kind="best-of", is_put=False)
    print(f"S0 {S0}: lower {d['lower']:.4f} ({d['se_lower']:.4f})  lattice {V:.4f}  upper {d['upper']:.4f} ({d['se_upper']:.4f})")
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)


def test_brackets_one_asset_with_a_dividend_yield(ctx):
    """d = 1 with q = 0.1: the American call that carries an early-exercise premium, against the one-asset lattice"""
    p = _params(is_put=False, N=9, M=100_000, T=3.0)
    d = ctx.price_american_basket_bounds(p, _ffi.make_basket([100.0], [0.2], [0.1], [1.0]), policy="textbook", **BIG)
    V = bl.one_asset(100.0, K, R, 0.2, 3.0, 9, 200, q=0.1, is_put=False)
    euro = bl.one_asset(100.0, K, R, 0.2, 3.0, 1, 1800, q=0.1, is_put=False)
    print(f"lower {d['lower']:.4f} ({d['se_lower']:.4f})  lattice {V:.4f} (european {euro:.4f})  upper {d['upper']:.4f} "
          f"({d['se_upper']:.4f})")
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)
    assert V > euro and d["n_exercised_lower"] > 0  # there is a premium, and the policy takes it


# ------------------------------------------------------------------ 5. known answers
SMALL = dict(n_lower=100_000, n_outer=1024, n_inner=128)


@pytest.mark.parametrize("kind", bc.KINDS)
def test_one_date_has_nothing_to_decide(ctx, kind):
    d = ctx.price_american_basket_bounds(_params(is_put=kind != "best-of", N=1), _basket(3, kind), **SMALL)
    assert d["n_exercised_lower"] == 0
    assert d["inner_path_steps"] == SMALL["n_outer"] * SMALL["n_inner"]
    assert abs(d["lower"] - d["upper"]) <= 4 * math.hypot(d["se_lower"], d["se_upper"]), d


def test_never_exercise_table(ctx):
    N = 10
    d = ctx.price_american_basket_bounds(_params(N=N), _basket(3, "basket"), policy="given", betas=np.zeros((N + 1, 4)),
                                         **SMALL)
    assert d["inner_path_steps"] == SMALL["n_outer"] * SMALL["n_inner"] * N * (N + 1) // 2
    assert d["n_exercised_lower"] == 0 and d["upper"] >= d["lower"]


# ------------------------------------------------------------------ 6. determinism, the float64 fallback
def test_deterministic_and_table_fallback(ctx):
    p, bk = _params(N=20, M=20_000), _basket(3, "worst-of")
    kw = dict(n_lower=50_000, n_outer=512, n_inner=200, want_q=True, want_samples=True)
    a = ctx.price_american_basket_bounds(p, bk, **kw)
    b = ctx.price_american_basket_bounds(p, bk, **kw)
    # every other step decided by the float64 rule instead of the tables: the same decisions, the same bits
    ctx.set_option("pass2_tables_irregular_every", 2)
    try:
        c = ctx.price_american_basket_bounds(p, bk, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    assert a["n_exercised_lower"] > 0
    for x in (b, c):
        for k in ("lower", "se_lower", "upper", "se_upper", "n_exercised_lower", "inner_path_steps"):
            assert x[k] == a[k], k
        for k in ("q", "samples", "betas"):
            np.testing.assert_array_equal(x[k], a[k])


# ------------------------------------------------------------------ 7. refusals
def _rc(ctx, p, b, policy=1, n_lower=1000, n_outer=64, n_inner=64, betas=None):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.BasketBounds()
    t = None if betas is None else np.ascontiguousarray(betas, np.float64)
    return ctx.lib.omc_price_american_basket_bounds(ctx.handle, C.byref(p), C.byref(b), C.byref(cfg),
                                                    t.ctypes.data if t is not None else None, None, None, None, C.byref(out))


def test_refusals(ctx):
    p, b = _params(), _basket(2, "best-of")
    assert _rc(ctx, _params(model="heston"), b) == -12
    assert _rc(ctx, p, _basket(2, "geometric")) == -34
    assert _rc(ctx, p, b, n_inner=63) == -3
    assert _rc(ctx, p, b, n_outer=63) == -3
    assert _rc(ctx, p, b, n_lower=999) == -3
    assert _rc(ctx, p, b, policy=7) == -4
    assert _rc(ctx, p, b, policy=3) == -7  # given without a table
    assert _rc(ctx, _params(N=252), b, n_outer=1 << 14, n_inner=1 << 12) == -16
    bad = _ffi.make_basket([100.0, 100.0], [0.2, 0.2], None, None, np.array([[1.0, 1.0], [1.0, 1.0]]), "best-of")
    assert _rc(ctx, p, bad) == -31  # a basket code passes through: rho is not positive definite
    assert _rc(ctx, p, b) == 0
    with pytest.raises(ValueError):
        ctx.price_american_basket_bounds(p, b, policy="given", betas=np.zeros((5, 4)), n_lower=1000, n_outer=64, n_inner=64)
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _rc(hooked, p, b) == -10
    finally:
        hooked.close()


# ------------------------------------------------------------------ 8. the facade and the C example
FAC = dict(n_lower=50_000, n_outer=512, n_inner=128)


def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_basket_bounds

    S0, sig, q, w = [100.0, 95.0, 105.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03], [1.0, 1.05, 0.95]
    f = price_american_basket_bounds(S0, K, R, sig, 1.0, 20_000, 10, correlation=RHO3, weights=w, dividend_yields=q,
                                     kind="worst-of", option_type="put", seed=42, stream=5, ctx=ctx, **FAC)
    p = _params(N=10, M=20_000, stream=5, S0=S0[0], sigma=sig[0])
    d = ctx.price_american_basket_bounds(p, _ffi.make_basket(S0, sig, q, w, RHO3, "worst-of"), **FAC)
    assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                              d["se_upper"], d["inner_path_steps"])
    np.testing.assert_array_equal(f.betas, d["betas"])
    assert (f.index0, f.n_assets, f.kind, f.policy) == (d["index0"], 3, "worst-of", "textbook")
    assert set(f.timings_ms) == {"fit", "lower", "upper", "total"}
    with pytest.raises(ValueError):
        price_american_basket_bounds(S0, K, R, sig, 1.0, 20_000, 10, n_inner=255, ctx=ctx)


def test_geometric_facade_is_one_asset(ctx):
    from options_model_amd import price_american_basket_bounds

    S0, sig, q, w = [100.0, 95.0, 105.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03], [0.5, 0.3, 0.2]
    f = price_american_basket_bounds(S0, K, R, sig, 1.0, 20_000, 10, correlation=RHO3, weights=w, dividend_yields=q,
                                     kind="geometric", ctx=ctx, **FAC)
    p = _params(N=10, M=20_000, S0=S0[0], sigma=sig[0])
    G0, sigma_G, q_G = _ffi.basket_table(p, _ffi.make_basket(S0, sig, q, w, RHO3, "geometric"))[4]
    d = ctx.price_american_basket_bounds(p, _ffi.make_basket([G0], [sigma_G], [q_G], [1.0]), **FAC)
    assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                              d["se_upper"], d["inner_path_steps"])
    assert (f.n_assets, f.kind) == (1, "geometric") and f.index0 == pytest.approx(G0, rel=1e-15)


def test_c_example_prints_the_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_basket_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_basket_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "100", "100000", "1024", "128"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    p = _params(is_put=False, N=9, M=100_000, T=3.0)
    b = _ffi.make_basket([100.0, 100.0], [0.2, 0.2], [0.1, 0.1], [1.0, 1.0], None, "best-of")
    ref = ctx.price_american_basket_bounds(p, b, n_lower=100_000, n_outer=1024, n_inner=128)
    lo, up = (float(v) for v in re.search(r"bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
    assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
    assert re.search(r"inner path-steps \d+", out) and "kernels:" in out and "max-call on 2 assets" in out
    assert not math.isnan(lo)

"""Jump-diffusion paths (omc_price_american_jump, options_model_amd/csrc/omc_jump.hip).

What is compared, and how tightly (as tests/test_gpu_dividends.py uses it):
  * lambda = 0                               `base` is omc_price_american's result, key for key (folded storage too)
  * mu_j = sigma_j = 0, lambda > 0           the matrix is the vanilla generator's at drift r - q, bit for bit, and `base`
                                             is omc_price_american_div's on it, key for key
  * the matrix with jumps                    tests/helpers/jump_ref.apply on the vanilla DEVICE matrix at the drift rate rj,
                                             counts and jump normals from the C oracle's Philox: rel 2e-5 GBM, 5e-5 Heston,
                                             atol = rtol * the column's largest reference spot (n_steps <= 64); every column
                                             carries the vanilla bits before its own first jump
  * sharding                                 a call at pair_offset P0 writes the columns of a larger call, bit for bit
  * the price                                the C oracle's two-pass flow on the device's own matrix: counts identical,
                                             price rel 1e-9
  * known answers                            the European value of the device matrix within 4 standard errors (from pair
                                             means) of Merton's series; mean(e^{-rT} S_T) within 4 of S0 e^{-qT}
"""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import dividend_ref as dr
from helpers.call_catalogue import diff, flat
from helpers import jump_ref as jr
from oracle import cpu as orc
from options_model_amd import _ffi
from test_gpu_dividends import HES, K, KEYS, MODELS, R, RTOL, S0, SHAPES, SIG, T, bits, check_price, params

pytestmark = pytest.mark.gpu

MU, SJ, Q = -0.1, 0.15, 0.02


def lam_of(N):
    return min(8.0, 0.5 * N / T)


def vanilla_at(ctx, p, rate):
    """the vanilla generator's matrix at drift `rate`"""
    if p.model == 1:
        S = ctx.heston_paths(p.n_paths, p.n_steps, p.S0, rate, p.T, p.v0, p.kappa, p.theta, p.xi, p.rho, p.seed, p.stream,
                             p.pair_offset, scheme=p.heston_scheme)
    else:
        S = ctx.gbm_paths(p.n_paths, p.n_steps, p.S0, rate, p.sigma, p.T, p.seed, p.stream, p.pair_offset)
    out = S.to_host()
    S.free()
    return out


def priced(ctx, p, jump, q):
    """-> (result dict, the path matrix the call wrote)"""
    keep = ctx.empty((p.n_steps + 1, p.n_paths), np.float32)
    out = ctx.price_american_jump(p, jump, q, S_keep=keep)
    S = keep.to_host()
    keep.free()
    return out, S


@functools.lru_cache(maxsize=None)
def draws(n_pairs, n_steps, seed, stream, pair_offset, thr):
    """counts and jump normals of a case: they depend on the counters only, so the four models share them"""
    return jr.draws(orc.philox4x32_10, n_pairs, n_steps, seed, stream, pair_offset, np.array(thr, np.uint32))


# ------------------------------------------------------------------ 1. lambda = 0: omc_price_american
@pytest.mark.parametrize("M,N,folded", [(20_004, 37, 0), (131_072, 12, 1)])
def test_no_jumps_is_price_american_key_for_key(ctx, M, N, folded):
    for model, scheme in (("gbm", 0), ("heston", 1)):
        for is_put in (True, False):
            p = params(model, scheme, is_put=is_put, M=M, N=N)
            a = ctx.price_american(p)
            b = ctx.price_american_jump(p, (0.0, MU, SJ), 0.0)
            assert [a[k] for k in KEYS] == [b[k] for k in KEYS], (model, is_put)
            assert b["folded"] == (folded if model == "gbm" else 0)
            assert b["n_thresholds"] == 0 and b["drift_rate"] == p.r
            assert b["kappa"] == pytest.approx(math.exp(MU + SJ * SJ / 2.0) - 1.0, rel=1e-15)
    p = params(M=M, N=N)  # with a yield: the yield-only route of omc_price_american_div
    a, b = ctx.price_american_div(p, Q, []), ctx.price_american_jump(p, (0.0, 0.0, 0.0), Q)
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS] and b["folded"] == folded


# ------------------------------------------------------------------ 2. jumps of size 0: the vanilla bits
@pytest.mark.parametrize("model,scheme", MODELS)
@pytest.mark.parametrize("M,N", SHAPES[:4])
def test_jumps_of_size_zero_change_no_bit(ctx, model, scheme, M, N):
    p = params(model, scheme, M=M, N=N, seed=9, stream=1, pair_offset=12345)
    V = vanilla_at(ctx, p, p.r - Q)
    keep = ctx.empty((N + 1, M), np.float32)
    out = ctx.price_american_jump(p, (lam_of(N), 0.0, 0.0), Q, S_keep=keep)
    assert np.array_equal(bits(keep.to_host()), bits(V)), (model, scheme)
    assert out["folded"] == 0 and out["kappa"] == 0.0 and out["drift_rate"] == p.r - Q and out["n_thresholds"] > 0
    ref = ctx.price_american_div(p, Q, [], S_keep=keep)
    keep.free()
    assert [out[k] for k in KEYS] == [ref[k] for k in KEYS]


# ------------------------------------------------------------------ 3. + 5. restatement and price, every shape and model
@pytest.mark.parametrize("model,scheme", MODELS)
@pytest.mark.parametrize("M,N", SHAPES)
def test_matrix_matches_the_restatement_and_price_the_oracle(ctx, model, scheme, M, N):
    lam = lam_of(N)
    for is_put, stream, off in ((True, 2, 0), (False, 3, 777)):
        p = params(model, scheme, is_put=is_put, M=M, N=N, seed=77, stream=stream, pair_offset=off)
        thr, kappa, rj = _ffi.jump_table(p, (lam, MU, SJ), Q)
        out, S = priced(ctx, p, (lam, MU, SJ), Q)
        assert out["folded"] == 0 and out["n_paths"] == M and (out["kappa"], out["drift_rate"]) == (kappa, rj)
        assert out["n_thresholds"] == int((thr < (1 << 24)).sum())
        if is_put or M <= 5_000:  # (the restatement's Philox loop runs once per large shape)
            V = vanilla_at(ctx, p, rj)
            n, z = draws(M // 2, N, int(p.seed), int(p.stream), int(p.pair_offset), tuple(int(t) for t in thr))
            ref = jr.apply(V, n, z, MU, SJ)
            ok, worst = dr.close(S, ref, ref, RTOL[model])  # atol = rtol * the column's largest reference spot
            print(f"{model}/{scheme} {M}x{N} put={is_put}: worst error / bound {worst:.3f}, jump cells {(n > 0).mean():.4f}")
            assert ok, (model, M, N, worst)
            first = jr.first_jump_step(n)
            before = np.arange(N + 1)[:, None] < np.concatenate([first, first])[None, :]
            assert np.array_equal(bits(S)[before], bits(V)[before])
            assert not (n > 0).any() or not np.array_equal(bits(S), bits(V))
            if M >= 20_000:
                x = lam * p.T / N
                cells, want = n[1:].size, 1.0 - math.exp(-x)
                assert abs((n[1:] > 0).mean() - want) <= 4.0 * math.sqrt(want * (1.0 - want) / cells)
        check_price(out, S, p)


# ------------------------------------------------------------------ 4. sharding by counter
@pytest.mark.parametrize("model,scheme", [("gbm", 0), ("heston", 0)])
def test_a_pair_offset_writes_the_columns_of_a_larger_call(ctx, model, scheme):
    M, N, P0, Ms = 20_008, 31, 3_001, 4_004
    jump = (lam_of(N), MU, SJ)
    _, big = priced(ctx, params(model, scheme, M=M, N=N, seed=5, stream=6), jump, Q)
    _, part = priced(ctx, params(model, scheme, M=Ms, N=N, seed=5, stream=6, pair_offset=P0), jump, Q)
    cols = np.arange(P0, P0 + Ms // 2)
    assert np.array_equal(bits(part[:, :Ms // 2]), bits(big[:, cols]))
    assert np.array_equal(bits(part[:, Ms // 2:]), bits(big[:, cols + M // 2]))


# ------------------------------------------------------------------ determinism, S_keep, leading dimension
def test_keeping_the_matrix_changes_nothing_and_calls_repeat(ctx):
    p = params("gbm", 0, M=20_004, N=37)
    jump = (8.0, MU, SJ)
    a = ctx.price_american_jump(p, jump, Q)
    b, S = priced(ctx, p, jump, Q)
    c = ctx.price_american_jump(p, jump, Q)
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS] == [c[k] for k in KEYS]
    keep = ctx.empty((p.n_steps + 1, p.n_paths + 3), np.float32)  # an odd leading dimension: scalar-width stores
    d = ctx.price_american_jump(p, jump, Q, S_keep=keep)
    assert [a[k] for k in KEYS[5:]] == [d[k] for k in KEYS[5:]] and d["price"] == pytest.approx(a["price"], rel=1e-12)
    assert np.array_equal(bits(keep.to_host()[:, :p.n_paths]), bits(S))
    keep.free()


# ------------------------------------------------------------------ 6. known answers
LAWS = [(1.0, -0.1, 0.15), (8.0, -0.05, 0.1), (16.0, 0.02, 0.05)]


def pair_mean_and_se(x):
    pm = 0.5 * (x[:x.size // 2] + x[x.size // 2:])
    return pm.mean(), pm.std(ddof=1) / math.sqrt(pm.size)


@pytest.mark.parametrize("lam,mu,sj", LAWS)
def test_european_value_of_the_matrix_is_mertons_series(ctx, lam, mu, sj):
    M, N = 65_536, 16
    _, S = priced(ctx, params(M=M, N=N, seed=123, stream=8), (lam, mu, sj), Q)
    ST = S[N].astype(np.float64)
    for is_put in (True, False):
        pay = math.exp(-R * T) * np.maximum(K - ST if is_put else ST - K, 0.0)
        mean, se = pair_mean_and_se(pay)
        ref = jr.merton(S0, K, R, Q, SIG, T, lam, mu, sj, is_put)
        print(f"lambda={lam} put={is_put}: device {mean:.5f} +- {se:.5f}  merton {ref:.5f}  z {(mean - ref) / se:+.2f}")
        assert abs(mean - ref) <= 4.0 * se


@pytest.mark.parametrize("model,scheme", MODELS[:3])
@pytest.mark.parametrize("lam,mu,sj", LAWS)
def test_discounted_spot_is_a_martingale(ctx, model, scheme, lam, mu, sj):
    """a wrong compensator fails this.  Merton, and Bates on the two log-Euler schemes: their step has the conditional mean
    e^{rj dt} exactly.  Scheme 2 is left out because its arithmetic Euler step has the mean 1 + rj dt, so the vanilla
    scheme-2 matrix itself misses S0 e^{(r-q)T} by rj^2 T dt / 2 -- up to 0.5 % here, several of these standard errors."""
    M, N = 65_536, 16
    _, S = priced(ctx, params(model, scheme, M=M, N=N, seed=321, stream=9), (lam, mu, sj), Q)
    mean, se = pair_mean_and_se(math.exp(-R * T) * S[N].astype(np.float64))
    want = S0 * math.exp(-Q * T)
    print(f"{model}/{scheme} lambda={lam}: device {mean:.5f} +- {se:.5f}  S0 e^-qT {want:.5f}  z {(mean - want) / se:+.2f}")
    assert abs(mean - want) <= 4.0 * se


# ------------------------------------------------------------------ 7. surfaces, refusals
def test_facade_returns_the_ffi_numbers(ctx):
    from options_model_amd import JumpResult, price_american_jumps
    for model in ("GBM", "Heston"):
        for opt in ("put", "call"):
            r = price_american_jumps(S0, K, R, SIG, T, 20_004, 37, 4.0, jump_mean=MU, jump_vol=SJ, dividend_yield=0.01,
                                     model=model, option_type=opt, seed=5)
            p = _ffi.make_params(model=model.lower(), is_put=(opt == "put"), semantics="two_pass", n_paths=20_004, n_steps=37,
                                 S0=S0, K=K, r=R, sigma=SIG, T=T, seed=5, v0=SIG ** 2, kappa=2.0, theta=SIG ** 2, xi=0.3, rho=-0.7)
            o = ctx.price_american_jump(p, (4.0, MU, SJ), 0.01)
            assert isinstance(r, JumpResult) and float(r) == r.price == o["price"]
            assert (r.n_exercised, r.sum_nitm, r.n_paths, r.folded) == (o["n_exercised"], o["sum_nitm"], 20_004, False)
            assert (r.kappa, r.drift_rate, r.info["max_jumps_per_step"]) == (o["kappa"], o["drift_rate"], o["n_thresholds"])
            assert r.stderr == math.sqrt(max(o["sumsq"] / 20_004 - o["price"] ** 2, 0.0) / 20_004)
    y = price_american_jumps(S0, K, R, SIG, T, 131_072, 12, 0.0, dividend_yield=0.03)
    assert y.folded and y.info["max_jumps_per_step"] == 0


def test_c_example_prints_the_same_price(tmp_path, ctx):
    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_jumps"
    subprocess.run(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "american_jumps.c"),
                    "-o", str(exe), "-L", os.path.dirname(lib), "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)],
                   check=True)
    out = subprocess.run([str(exe), "200000", "50"], check=True, capture_output=True, text=True).stdout
    for name, model, lam in (("merton, lambda 1", "gbm", 1.0), ("bates, lambda 1", "heston", 1.0), ("gbm, no jumps", "gbm", 0.0)):
        price = float(re.search(re.escape(name) + r": price ([0-9.]+)", out).group(1))
        p = _ffi.make_params(model=model, semantics="two_pass", n_paths=200000, n_steps=50, seed=42, **HES)
        ref = ctx.price_american_jump(p, (lam, -0.1, 0.15), 0.02)
        assert abs(price - ref["price"]) < 1e-6, name


def test_invalid_arguments_raise_and_the_context_still_prices(ctx):
    import ctypes as C
    p = params(M=4096, N=20)
    before = flat(ctx.price_american_jump(p, (1.0, MU, SJ), Q))
    for jump, q in (((-1.0, 0.0, 0.0), 0.0), ((1.0, math.nan, 0.0), 0.0), ((1.0, 0.0, -0.1), 0.0), ((20.5, 0.0, 0.0), 0.0),
                    ((1.0, 0.0, 0.0), math.inf)):
        with pytest.raises(ValueError):
            ctx.price_american_jump(p, jump, q)
    for bad in (params(M=4096, N=20, antithetic=False), _ffi.make_params(semantics="reference", n_paths=4096, n_steps=20)):
        with pytest.raises(ValueError):
            ctx.price_american_jump(bad, (1.0, MU, SJ), 0.0)
    keep = ctx.empty((21, 4000), np.float32)
    with pytest.raises(ValueError):  # -6: leading dimension below n_paths
        ctx.price_american_jump(p, (1.0, MU, SJ), 0.0, S_keep=keep)
    keep.free()
    out = _ffi.JumpResult()
    assert ctx.lib.omc_price_american_jump(ctx.handle, C.byref(p), None, 0.0, C.byref(out), None, 0) == -25
    assert ctx.lib.omc_price_american_jump(ctx.handle, C.byref(p), C.byref(_ffi.Jump(1.0, MU, SJ)), 0.0, None, None, 0) == -7
    c = _ffi.Context(0)
    try:
        c.set_allreduce_hook(lambda dptr, count: None)
        assert c.lib.omc_price_american_jump(c.handle, C.byref(p), C.byref(_ffi.Jump(1.0, MU, SJ)), 0.0, C.byref(out), None, 0) == -10
        c.set_allreduce_hook(None)
        assert not diff(flat(c.price_american_jump(p, (1.0, MU, SJ), Q)), before)
    finally:
        c.close()
    assert not diff(flat(ctx.price_american_jump(p, (1.0, MU, SJ), Q)), before)

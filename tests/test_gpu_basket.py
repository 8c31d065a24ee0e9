"""Multi-asset options (omc_price_american_basket, options_model_amd/csrc/omc_basket.hip).

What is compared, and how tightly (as tests/test_gpu_dividends.py uses it):
  * d = 1, w = 1, any kind                   the index matrix is the vanilla generator's at rate r - q, bit for bit, and
                                             `base` is omc_price_american_div's on it, key for key
  * rho = I                                  asset k's matrix is the vanilla generator's at (S0_k, r - q_k, sigma_k) and pair
                                             offset pair_offset + (k << 40), bit for bit; with any rho asset 0's still is
  * correlated assets                        tests/helpers/basket_ref.assets on the C oracle's normals at the tagged offsets:
                                             rel 2e-5, atol = rtol * the column's largest reference spot (n_steps <= 64)
  * the index                                the restatement on the DEVICE's own asset matrices: best-of / worst-of bit for
                                             bit, arithmetic rel d 2^-23 (one rounding per term of the chain), geometric rel
                                             2e-5 (N roundings of exp2)
  * the price                                the C oracle's two-pass flow on the device's own index matrix: counts
                                             identical, price rel 1e-9
  * sharding                                 a call at pair_offset P0 writes the columns of a larger call, bit for bit
  * known answers                            within 4 standard errors (from pair means): the discounted arithmetic index,
                                             the cross moments E[S_i S_j], the European value of the geometric index
  * the American geometric basket            8 seeds against 8 one-dimensional pricings at (G0, sigma_G, q_G): Welch |t| <= 4
"""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import basket_ref as br
from helpers import dividend_ref as dr
from helpers.call_catalogue import diff, flat
from oracle import cpu as orc
from options_model_amd import _ffi
from test_gpu_dividends import K, KEYS, R, SHAPES, T, bits, check_price, params

pytestmark = pytest.mark.gpu

KINDS = ("basket", "geometric", "best-of", "worst-of")
RTOL = 2e-5


def equi(d, c):
    return np.full((d, d), c) + (1.0 - c) * np.eye(d)


RHO3 = np.array([[1.0, 0.5, 0.2], [0.5, 1.0, -0.3], [0.2, -0.3, 1.0]])
# (S0, sigma, q, weights of the basket kinds, weights of best-of / worst-of, rho)
CASE3 = ([100.0, 95.0, 105.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03], [0.5, 0.3, 0.2], [1.0, 1.05, 0.95], RHO3)
CASE8 = ([90.0 + 3.0 * i for i in range(8)], [0.15 + 0.02 * i for i in range(8)], [0.005 * i for i in range(8)],
         [0.06 + 0.02 * i for i in range(8)], [1.1 - 0.02 * i for i in range(8)], equi(8, 0.3))


def basket_of(case, kind, rho=None):
    S0, sig, q, w_sum, w_max, rho_c = case
    w = w_sum if kind in ("basket", "geometric") else w_max
    return _ffi.make_basket(S0, sig, q, w, rho_c if rho is None else rho, kind), w


def priced(ctx, p, b, pad=0, assets=True):
    """-> (result dict, the index matrix, the asset matrices [d][N+1][M]) with the leading dimension n_paths + pad"""
    d, ld = int(b.n_assets), p.n_paths + pad
    keep = ctx.empty((p.n_steps + 1, ld), np.float32)
    akeep = ctx.empty((d, p.n_steps + 1, ld), np.float32) if assets else None
    out = ctx.price_american_basket(p, b, S_keep=keep, assets_keep=akeep)
    S = keep.to_host()[:, :p.n_paths]
    A = akeep.to_host()[:, :, :p.n_paths] if assets else None
    keep.free()
    if assets:
        akeep.free()
    return out, S, A


def vanilla(ctx, p, S0, rate, sigma, tag=0):
    V = ctx.gbm_paths(p.n_paths, p.n_steps, S0, rate, sigma, p.T, p.seed, p.stream, p.pair_offset + (tag << 40))
    out = V.to_host()
    V.free()
    return out


def pair_mean_and_se(x):
    pm = 0.5 * (x[:x.size // 2] + x[x.size // 2:])
    return pm.mean(), pm.std(ddof=1) / math.sqrt(pm.size)


# ------------------------------------------------------------------ 1. one asset of weight 1: the vanilla pricing
@pytest.mark.parametrize("M,N", SHAPES)
def test_one_asset_is_the_vanilla_matrix_and_the_dividend_pricing(ctx, M, N):
    S0, sig, q = 93.0, 0.27, 0.02
    for i, kind in enumerate(KINDS):
        p = params(is_put=(i % 2 == 0), M=M, N=N, seed=9, stream=1, pair_offset=12345, S0=S0, sigma=sig)
        out, S, A = priced(ctx, p, _ffi.make_basket([S0], [sig], [q], [1.0], kind=kind))
        V = vanilla(ctx, p, S0, p.r - q, sig)
        assert np.array_equal(bits(S), bits(V)) and np.array_equal(bits(A[0]), bits(V)), kind
        keep = ctx.empty((N + 1, M), np.float32)
        ref = ctx.price_american_div(p, q, [], S_keep=keep)
        keep.free()
        assert [out[k] for k in KEYS] == [ref[k] for k in KEYS], kind
        assert (out["n_assets"], out["kind"], out["index0"], out["folded"]) == (1, i, S0, 0)


# ------------------------------------------------------------------ 2. rho = I: every asset is a vanilla matrix
@pytest.mark.parametrize("d", [2, 3, 4, 8])
@pytest.mark.parametrize("M,N", SHAPES)
def test_identity_correlation_gives_the_vanilla_matrix_per_asset(ctx, M, N, d):
    S0, sig, q, w, _, _ = CASE8
    b = _ffi.make_basket(S0[:d], sig[:d], q[:d], w[:d], np.eye(d), "basket")
    p = params(M=M, N=N, seed=21, stream=2, pair_offset=777)
    V = [vanilla(ctx, p, S0[k], p.r - q[k], sig[k], tag=k) for k in range(d)]
    for pad in (0, 3):  # 3: an odd leading dimension, scalar-width stores
        _, S, A = priced(ctx, p, b, pad=pad)
        for k in range(d):
            assert np.array_equal(bits(A[k]), bits(V[k])), (k, pad)
        ref = br.index(A, w[:d], "basket")
        assert np.abs(S / ref - 1.0).max() <= d * 2.0 ** -23


# ------------------------------------------------------------------ 3. + 4. correlated assets, the index, the price
@pytest.mark.parametrize("case", [CASE3, CASE8], ids=["3-assets", "8-assets"])
@pytest.mark.parametrize("M,N", SHAPES)
def test_assets_index_and_price_match_restatement_and_oracle(ctx, M, N, case):
    S0, sig, q = case[:3]
    d = len(S0)
    ref_assets = None
    for i, kind in enumerate(KINDS):
        b, w = basket_of(case, kind)
        for is_put, stream, off in ((True, 2, 4321), (False, 3, (1 << 33) + 5)):
            p = params(is_put=is_put, M=M, N=N, seed=77, stream=stream, pair_offset=off)
            L, a, bb, x0, geo = _ffi.basket_table(p, b)
            out, S, A = priced(ctx, p, b, assets=is_put)
            assert (out["folded"], out["n_paths"], out["n_assets"], out["kind"], out["index0"]) == (0, M, d, i, x0)
            if is_put and ref_assets is None:  # the assets depend on neither the kind nor the side: compared once per shape
                z = [orc.gbm_normals(M // 2, N, int(p.seed), int(p.stream), int(p.pair_offset) + (k << 40)) for k in range(d)]
                ref_assets = br.assets(z, S0, a, bb, L)
                for k in range(d):
                    ok, worst = dr.close(A[k], ref_assets[k], ref_assets[k], RTOL)
                    print(f"{d} assets {M}x{N}: asset {k} worst error / bound {worst:.3f}")
                    assert ok, (k, worst)
                    assert k == 0 or not np.array_equal(bits(A[k]), bits(vanilla(ctx, p, S0[k], p.r - q[k], sig[k], tag=k)))
            if is_put:  # the index from the device's own asset matrices
                assert np.array_equal(bits(A[0]), bits(vanilla(ctx, p, S0[0], p.r - q[0], sig[0]))), kind  # whatever rho is
                ref = br.index(A, w, kind, S0=S0, G0=geo[0])
                if kind in ("best-of", "worst-of"):
                    assert np.array_equal(bits(S), bits(ref)), kind
                else:
                    err = np.abs(S / ref - 1.0).max()
                    print(f"{d} assets {M}x{N} {kind}: index rel error {err:.3e}")
                    assert err <= (d * 2.0 ** -23 if kind == "basket" else RTOL), (kind, err)
            check_price(out, S, p)


# ------------------------------------------------------------------ 5. sharding by counter, S_keep, determinism
@pytest.mark.parametrize("kind", ["basket", "geometric"])
def test_a_pair_offset_writes_the_columns_of_a_larger_call(ctx, kind):
    M, N, P0, Ms = 20_008, 31, 3_001, 4_004
    b, _ = basket_of(CASE3, kind)
    _, big, bigA = priced(ctx, params(M=M, N=N, seed=5, stream=6, pair_offset=11), b)
    _, part, partA = priced(ctx, params(M=Ms, N=N, seed=5, stream=6, pair_offset=11 + P0), b)
    cols = np.arange(P0, P0 + Ms // 2)
    assert np.array_equal(bits(part[:, :Ms // 2]), bits(big[:, cols]))
    assert np.array_equal(bits(part[:, Ms // 2:]), bits(big[:, cols + M // 2]))
    assert np.array_equal(bits(partA[:, :, :Ms // 2]), bits(bigA[:, :, cols]))
    assert np.array_equal(bits(partA[:, :, Ms // 2:]), bits(bigA[:, :, cols + M // 2]))


def test_keeping_the_matrices_changes_nothing_and_calls_repeat(ctx):
    p = params(M=20_004, N=37)
    for kind in KINDS:
        b, _ = basket_of(CASE3, kind)
        a = ctx.price_american_basket(p, b)
        bo, S, A = priced(ctx, p, b)
        c, S2, _ = priced(ctx, p, b, assets=False)
        akeep = ctx.empty((3, p.n_steps + 1, p.n_paths), np.float32)
        d = ctx.price_american_basket(p, b, assets_keep=akeep)  # the assets alone: the index stays in the library's matrix
        A2 = akeep.to_host()
        akeep.free()
        e = ctx.price_american_basket(p, b)
        assert [a[k] for k in KEYS] == [bo[k] for k in KEYS] == [c[k] for k in KEYS] == [d[k] for k in KEYS] == [e[k] for k in KEYS]
        assert np.array_equal(bits(S), bits(S2)) and np.array_equal(bits(A), bits(A2))


# ------------------------------------------------------------------ 6. known answers
def test_known_moments_and_the_european_geometric_value(ctx):
    M, N = 65_536, 16
    S0, sig, q = [100.0, 95.0, 105.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03]
    w = [0.5, 0.3, 0.2]
    rho = np.array([[1.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 1.0]])
    p = params(M=M, N=N, seed=123, stream=8)
    _, S, A = priced(ctx, p, _ffi.make_basket(S0, sig, q, w, rho, "basket"))
    mean, se = pair_mean_and_se(math.exp(-R * T) * S[N].astype(np.float64))
    want = sum(w[i] * S0[i] * math.exp(-q[i] * T) for i in range(3))
    print(f"discounted arithmetic index: device {mean:.5f} +- {se:.5f}  exact {want:.5f}  z {(mean - want) / se:+.2f}")
    assert abs(mean - want) <= 4.0 * se
    AT = A[:, N].astype(np.float64)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        mean, se = pair_mean_and_se(AT[i] * AT[j])
        want = S0[i] * S0[j] * math.exp((2.0 * R - q[i] - q[j] + rho[i, j] * sig[i] * sig[j]) * T)
        print(f"E[S_{i} S_{j}]: device {mean:.3f} +- {se:.3f}  exact {want:.3f}  z {(mean - want) / se:+.2f}")
        assert abs(mean - want) <= 4.0 * se
    b = _ffi.make_basket(S0, sig, q, w, rho, "geometric")
    _, _, _, _, (G0, sG, qG) = _ffi.basket_table(p, b)
    _, G, _ = priced(ctx, p, b, assets=False)
    GT = G[N].astype(np.float64)
    for is_put in (True, False):
        mean, se = pair_mean_and_se(math.exp(-R * T) * np.maximum(K - GT if is_put else GT - K, 0.0))
        want = dr.bsm(G0, K, R, qG, sG, T, is_put)
        print(f"european geometric put={is_put}: device {mean:.5f} +- {se:.5f}  bsm {want:.5f}  z {(mean - want) / se:+.2f}")
        assert abs(mean - want) <= 4.0 * se


# ------------------------------------------------------------------ 7. the American geometric basket is one-dimensional
@pytest.mark.parametrize("is_put", [True, False])
def test_american_geometric_basket_is_the_one_dimensional_option(ctx, is_put):
    """Two samples of 8 pricings compared by Welch's t: the seed-to-seed scatter of these in-sample estimates is 1 - 2
    times a single pricing's own standard error, so single pricings are not compared by it."""
    M, N = 65_536, 16
    b, _ = basket_of(CASE3, "geometric")
    G0, sG, qG = _ffi.basket_table(params(M=M, N=N), b)[4]
    keep = ctx.empty((N + 1, M), np.float32)
    multi = [ctx.price_american_basket(params(is_put=is_put, M=M, N=N, seed=100 + s, stream=4), b)["price"] for s in range(8)]
    one = [ctx.price_american_div(params(is_put=is_put, M=M, N=N, seed=200 + s, stream=4, S0=G0, sigma=sG), qG, [],
                                  S_keep=keep)["price"] for s in range(8)]
    keep.free()
    m1, m2, v1, v2 = np.mean(multi), np.mean(one), np.var(multi, ddof=1), np.var(one, ddof=1)
    t = (m1 - m2) / math.sqrt(v1 / 8 + v2 / 8)
    print(f"put={is_put}: basket {m1:.4f} (sd {math.sqrt(v1):.4f})  one-dimensional {m2:.4f} (sd {math.sqrt(v2):.4f})  t {t:+.2f}")
    assert abs(t) <= 4.0


# ------------------------------------------------------------------ 8. surfaces, refusals
def test_facade_returns_the_ffi_numbers(ctx):
    from options_model_amd import BasketResult, price_american_basket
    S0, sig, q, w_sum, _, rho = CASE3
    for kind in KINDS:
        for opt in ("put", "call"):
            r = price_american_basket(S0, K, R, sig, T, 20_004, 37, correlation=rho, dividend_yields=q, kind=kind,
                                      option_type=opt, seed=5)
            w = [1.0 / 3] * 3 if kind in ("basket", "geometric") else [1.0] * 3
            p = _ffi.make_params(is_put=(opt == "put"), semantics="two_pass", n_paths=20_004, n_steps=37, K=K, r=R, T=T, seed=5)
            o = ctx.price_american_basket(p, _ffi.make_basket(S0, sig, q, w, rho, kind))
            assert isinstance(r, BasketResult) and float(r) == r.price == o["price"]
            assert (r.n_exercised, r.sum_nitm, r.n_paths, r.index0, r.n_assets, r.kind) == \
                (o["n_exercised"], o["sum_nitm"], 20_004, o["index0"], 3, kind)
            assert r.stderr == math.sqrt(max(o["sumsq"] / 20_004 - o["price"] ** 2, 0.0) / 20_004) and r.info["weights"] == w
    # the defaults: identity correlation, no yields, seed 42; explicit weights
    r = price_american_basket([100.0, 110.0], K, R, [0.2, 0.3], T, 4_096, 20, weights=[0.7, 0.2])
    p = _ffi.make_params(semantics="two_pass", n_paths=4_096, n_steps=20, K=K, r=R, T=T, seed=42)
    assert r.price == ctx.price_american_basket(p, _ffi.make_basket([100.0, 110.0], [0.2, 0.3], None, [0.7, 0.2]))["price"]
    assert r.index0 == pytest.approx(92.0, rel=1e-15)


def test_c_example_prints_the_same_prices(tmp_path, ctx):
    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_basket"
    subprocess.run(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "american_basket.c"),
                    "-o", str(exe), "-L", os.path.dirname(lib), "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)],
                   check=True)
    out = subprocess.run([str(exe), "200000", "50"], check=True, capture_output=True, text=True).stdout
    cases = (("basket put, 3 assets", True, _ffi.make_basket(*CASE3[:4], RHO3, "basket")),
             ("best-of call, 2 assets", False, _ffi.make_basket([100.0, 95.0], [0.2, 0.3], [0.02, 0.04], [1.0, 1.0],
                                                                [[1.0, 0.6], [0.6, 1.0]], "best-of")),
             ("basket put, 1 asset", True, _ffi.make_basket([100.0], [0.2], [0.02], [1.0])))
    for name, is_put, b in cases:
        price = float(re.search(re.escape(name) + r": price ([0-9.]+)", out).group(1))
        p = _ffi.make_params(is_put=is_put, semantics="two_pass", n_paths=200000, n_steps=50, K=100.0, r=0.05, T=1.0, seed=42)
        assert abs(price - ctx.price_american_basket(p, b)["price"]) < 1e-6, name


def test_invalid_arguments_raise_and_the_context_still_prices(ctx):
    import ctypes as C
    p = params(M=4096, N=20)
    good, _ = basket_of(CASE3, "basket")
    before = flat(ctx.price_american_basket(p, good))
    npd = [[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]]
    for bad in (_ffi.make_basket([100.0, -1.0], [0.2, 0.2]), _ffi.make_basket([100.0, 90.0], [0.2, 0.0]),
                _ffi.make_basket([100.0, 90.0], [0.2, 0.2], weights=[1.0, 0.0]),
                _ffi.make_basket([100.0, 90.0], [0.2, 0.2], yields=[0.0, math.nan]),
                _ffi.make_basket([100.0] * 3, [0.2] * 3, correlation=npd), _ffi.make_basket([100.0, 90.0], [0.2, 0.2], kind=9)):
        with pytest.raises(ValueError):
            ctx.price_american_basket(p, bad)
    for badp in (params(M=4096, N=20, antithetic=False), _ffi.make_params(semantics="reference", n_paths=4096, n_steps=20),
                 params("heston", 0, M=4096, N=20), params(M=4096, N=20, pair_offset=(1 << 40) - 2047)):
        with pytest.raises(ValueError):
            ctx.price_american_basket(badp, good)
    keep, akeep = ctx.empty((21, 4000), np.float32), ctx.empty((3, 21, 4000), np.float32)
    with pytest.raises(ValueError):  # -6: leading dimension below n_paths
        ctx.price_american_basket(p, good, S_keep=keep)
    with pytest.raises(ValueError):
        ctx.price_american_basket(p, good, assets_keep=akeep)
    keep.free()
    akeep.free()
    out = _ffi.BasketResult()
    lib = ctx.lib
    assert lib.omc_price_american_basket(ctx.handle, C.byref(p), None, C.byref(out), None, None, 0) == -29
    assert lib.omc_price_american_basket(ctx.handle, C.byref(p), C.byref(good), None, None, None, 0) == -7
    assert lib.omc_price_american_basket(ctx.handle, C.byref(params(M=4096, N=20, pair_offset=(1 << 40) - 2047)), C.byref(good),
                                         C.byref(out), None, None, 0) == -33
    c = _ffi.Context(0)
    try:
        c.set_allreduce_hook(lambda dptr, count: None)
        assert c.lib.omc_price_american_basket(c.handle, C.byref(p), C.byref(good), C.byref(out), None, None, 0) == -10
        c.set_allreduce_hook(None)
        assert not diff(flat(c.price_american_basket(p, good)), before)
    finally:
        c.close()
    assert not diff(flat(ctx.price_american_basket(p, good)), before)

"""The Heston QE scheme on the device (OMC_HESTON_QE = 3; include/omc.h).

What is compared, and how tightly:
  * the generator                      per spot against the float64 restatement (tests/helpers/heston_qe_ref.py) on the
                                       device's own normals: rel 5e-5 of the column's largest spot (the project's Heston
                                       bound for n_steps <= 64).  Columns with a step inside one of the rule's two
                                       discontinuity bands are left out (at most 1 % per case) and may deviate only from that
                                       step on
  * shared code                        the sv generator, a restart from (S_t, V_t), a pair offset: bit for bit
  * European sums, surface             the stored last row to 1e-12; the surface against its per-expiry calls bit for bit
  * barrier / dividend / jump          an untouched barrier, a zero dividend, zero jumps: the vanilla matrix bit for bit
  * the American price, the Greeks     the C oracle's two-pass flow on the device's matrix: counts equal, price 1e-9
  * known answers                      Andersen's Case I at quarter-year steps against the semi-analytic price
The consumers with work to do (a barrier that is met, real dividends and jumps): tests/test_gpu_heston_qe_consumers.py.
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import heston_qe_ref as qe
from oracle import cpu as orc
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

QE, FT = 3, 1
S0, R, T = qe.MARKET["S0"], qe.MARKET["r"], qe.MARKET["T"]
K = 100.0
KEYS = ("price", "sum", "sumsq", "std", "zero_prob", "n_paths", "n_exercised", "n_zero", "sum_nitm", "folded")


def host(a):
    h = a.to_host()
    a.free()
    return h


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hp_list(hp):
    return [hp[k] for k in ("v0", "kappa", "theta", "xi", "rho")]


def paths(ctx, hp, M, N, seed=qe.SEED, stream=qe.STREAM, off=0, scheme=QE, s0=S0, r=R, t=T):
    return host(ctx.heston_paths(M, N, s0, r, t, *hp_list(hp), seed, stream, off, scheme))


def paths_sv(ctx, hp, M, N, seed=qe.SEED, stream=qe.STREAM, off=0, scheme=QE):
    Sd, Vd = ctx.heston_paths_sv(M, N, S0, R, T, *hp_list(hp), seed, stream, off, scheme)
    return host(Sd), host(Vd)


def normals(ctx, H, N, seed=qe.SEED, stream=qe.STREAM, off=0):
    return qe.pair_view(host(ctx.gbm_normals(H, 2 * N, seed, stream, off)))


def params(hp, M, N, is_put=True, scheme=QE, seed=qe.SEED, stream=qe.STREAM, off=0, **kw):
    kw = {**dict(S0=S0, K=K, r=R, T=T), **kw}
    return _ffi.make_params(model="heston", heston_scheme=scheme, is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N,
                            sigma=0.0, seed=seed, stream=stream, pair_offset=off, **kw, **hp)


# ---------------------------------------------------------------------------------------------- 1. accepted
@pytest.mark.parametrize("name", list(qe.SETS))
def test_scheme_three_is_accepted(ctx, name):
    hp = qe.SETS[name]
    M, N = 2 * 257, 7
    S = ctx.empty((N + 1, M), np.float32)
    try:
        rc = ctx.lib.omc_heston_paths_f32(ctx.handle, S.ptr, M, M, N, S0, R, T, *hp_list(hp), qe.SEED, qe.STREAM, 0, QE)
        assert rc == 0, (rc, ctx.last_error() if hasattr(ctx, "last_error") else "")
        X = S.to_host()
    finally:
        S.free()
    assert np.all(X[0] == np.float32(S0)) and np.isfinite(X).all() and X.min() > 0.0
    S2, V = paths_sv(ctx, hp, M, N)
    assert np.isfinite(V).all() and V.min() >= 0.0 and np.all(V[0] == np.float32(hp["v0"]))
    assert np.array_equal(bits(S2), bits(X))
    assert np.any(V[1:, :M // 2] != V[1:, M // 2:])  # the partners' variances are their own


# ---------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("name", list(qe.SETS))
def test_device_against_the_restatement_per_spot(ctx, name):
    hp = qe.SETS[name]
    worst = share = 0.0
    for H in qe.PAIR_COUNTS:
        for N in qe.STEP_COUNTS:
            z1, z2 = normals(ctx, H, N)
            ref = qe.paths(z1, z2, S0, hp["v0"], R, T, hp["kappa"], hp["theta"], hp["xi"], hp["rho"])
            got = qe.compare(paths(ctx, hp, 2 * H, N), ref, qe.RTOL)
            print(f"set {name} pairs {H} steps {N}: worst {got['worst']:.3e} left out {got['share']:.4f}")
            assert got["share"] <= qe.MAX_SHARE, (name, H, N, got)
            worst, share = max(worst, got["worst"]), max(share, got["share"])
            if name == "A":
                assert not ref["expo"].any()
            if name == "C":
                assert ref["expo"][0].all()
    print(f"set {name}: worst deviation {worst:.3e} of the column's largest spot, largest share left out {share:.4f}")


# ---------------------------------------------------------------------------------------------- 3. shared code
@pytest.mark.parametrize("name", list(qe.SETS))
@pytest.mark.parametrize("M,N", [(2048, 64), (514, 7), (130, 3), (2, 1)])
def test_sv_generator_keeps_the_spots_bits(ctx, name, M, N):
    hp = qe.SETS[name]
    S2, V = paths_sv(ctx, hp, M, N, off=3)
    assert np.array_equal(bits(S2), bits(paths(ctx, hp, M, N, off=3)))
    assert V.min() >= 0.0


@pytest.mark.parametrize("name", list(qe.SETS))
def test_sv_state_restarts_the_path(ctx, name):
    """tests/test_gpu_heston_bounds.py's restart property at scheme 3: from (S[t, j], V[t, j]) and the generator's remaining
    normals the from-normals entry point gives rows t + 1 .. N of that column bit for bit, for both partners (each from ITS
    state: the first output column is the pair's first partner, the second its antithetic one)."""
    hp = qe.SETS[name]
    M, N, off = 1000, 13, 7
    P = M // 2
    S, V = paths_sv(ctx, hp, M, N, off=off)
    z1, z2 = normals(ctx, P, N, off=off)
    for t in (0, 4, 12):
        low = np.argsort(np.minimum(V[t, :P], V[t, P:]))[:4]  # the pairs with the lowest variance state at t
        for j in sorted({0, 1, P - 1, *[int(x) for x in low]}):
            pad1, pad2 = np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32)
            pad1[:N - t, 0], pad2[:N - t, 0] = z1[t:, j], z2[t:, j]
            for col, out_col in ((j, 0), (j + P, 1)):
                X = host(ctx.heston_paths_from_normals(pad1, pad2, float(S[t, col]), R, T, float(V[t, col]), hp["kappa"],
                                                       hp["theta"], hp["xi"], hp["rho"], QE))
                np.testing.assert_array_equal(bits(X[1:N - t + 1, out_col]), bits(S[t + 1:, col]),
                                              err_msg=f"set {name} t {t} column {col}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_pair_offset_writes_the_columns_of_a_larger_call(ctx, name):
    hp = qe.SETS[name]
    N, P, off, h = 9, 771, 2 ** 33 + 5, 257  # the shard starts at pair 257 of the larger call
    whole = paths(ctx, hp, 2 * P, N, off=off)
    part = paths(ctx, hp, 2 * (P - h), N, off=off + h)
    assert np.array_equal(bits(part[:, :P - h]), bits(whole[:, h:P]))
    assert np.array_equal(bits(part[:, P - h:]), bits(whole[:, P + h:]))


# ---------------------------------------------------------------------------------------------- 4. European sums
@pytest.mark.parametrize("name", ["A", "B"])
def test_european_sums_of_the_stored_last_row(ctx, name):
    hp = qe.SETS[name]
    df = math.exp(-R * T)
    for M, N in ((4098, 9), (514, 5), (2, 1), (66_000, 3)):
        ST = paths(ctx, hp, M, N, stream=5, off=11)[-1].astype(np.float64)
        for is_put in (True, False):
            pay = np.maximum(K - ST if is_put else ST - K, 0.0) * df
            res = ctx.price_european(params(hp, M, N, is_put=is_put, stream=5, off=11))
            assert abs(res["sum"] - math.fsum(pay)) <= 1e-12 * math.fsum(pay) + 1e-300, (M, N, is_put)
            assert abs(res["sumsq"] - math.fsum(pay * pay)) <= 1e-12 * math.fsum(pay * pay) + 1e-300
            assert res["n_zero"] == int(np.count_nonzero(pay == 0.0)) and res["n_paths"] == M
            one = ctx.price_european_batch([params(hp, M, N, is_put=is_put, stream=5, off=11)])[0]
            assert (one["sum"], one["sumsq"], one["n_zero"]) == (res["sum"], res["sumsq"], res["n_zero"])


def test_strike_prices_and_the_surface(ctx):
    """omc_heston_price_strikes at scheme 3 is the mean payoff of the stored generator's last row (same stream), and
    omc_heston_price_surface equals its per-expiry calls bit for bit"""
    hp = qe.SET_B
    M, N = 4098, 6
    strikes = np.array([80.0, 100.0, 125.0])
    prices, errs = ctx.heston_price_strikes(M, N, S0, R, T, *hp_list(hp), strikes, is_put=False, seed=qe.SEED, stream=4, scheme=QE)
    ST = paths(ctx, hp, M, N, stream=4)[-1].astype(np.float64)
    for k, x in enumerate(strikes):
        ref = math.exp(-R * T) * math.fsum(np.maximum(ST - x, 0.0)) / M
        assert abs(prices[k] - ref) <= 1e-12 * ref
    expiries, streams = np.array([0.25, 1.0, 2.0]), np.array([7, 8, 9], np.uint64)
    ks = np.array([90.0, 100.0, 110.0, 95.0, 105.0, 100.0])
    eo = np.array([0, 0, 1, 1, 2, 2], np.int32)
    sp, se = ctx.heston_price_surface(M, N, S0, R, *hp_list(hp), expiries, streams, ks, eo, is_put=True, seed=qe.SEED, scheme=QE)
    for e in range(3):
        m = eo == e
        p1, e1 = ctx.heston_price_strikes(M, N, S0, R, float(expiries[e]), *hp_list(hp), ks[m], is_put=True, seed=qe.SEED,
                                          stream=int(streams[e]), scheme=QE)
        assert np.array_equal(sp[m], p1) and np.array_equal(se[m], e1), e


# ---------------------------------------------------------------------------------------------- 5. exotic generators
EX_M, EX_N = 512, 7  # 256 pairs x 7 steps


def _kept(ctx, call):
    keep = ctx.empty((EX_N + 1, EX_M), np.float32)
    try:
        out = call(keep)
        return out, keep.to_host()
    finally:
        keep.free()


@pytest.mark.parametrize("name", ["A", "B"])
def test_exotic_generators_write_the_vanilla_matrix(ctx, name):
    hp = qe.SETS[name]
    p = params(hp, EX_M, EX_N)
    V = paths(ctx, hp, EX_M, EX_N)
    # a barrier that is never touched
    _, S = _kept(ctx, lambda keep: ctx.price_barrier(p, "down-and-out", 1e-6 * S0, keep_paths=keep))
    assert np.array_equal(bits(S), bits(V))
    # no dividends, and a dividend of amount zero (the dividend generator's own kernel)
    base = ctx.price_american(p)
    out, S = _kept(ctx, lambda keep: ctx.price_american_div(p, 0.0, [], S_keep=keep))
    assert np.array_equal(bits(S), bits(V)) and [out[k] for k in KEYS] == [base[k] for k in KEYS]
    out, S = _kept(ctx, lambda keep: ctx.price_american_div(p, 0.0, [(0.5 * T, 0.0, "cash")], S_keep=keep))
    assert np.array_equal(bits(S), bits(V)) and out["n_div_steps"] == 1
    # zero jump intensity, and jumps of size zero (the jump generator's own kernel, both sides of its ballot)
    out, S = _kept(ctx, lambda keep: ctx.price_american_jump(p, (0.0, -0.1, 0.15), 0.0, S_keep=keep))
    assert np.array_equal(bits(S), bits(V)) and [out[k] for k in KEYS] == [base[k] for k in KEYS]
    out, S = _kept(ctx, lambda keep: ctx.price_american_jump(p, (3.0, 0.0, 0.0), 0.0, S_keep=keep))
    assert np.array_equal(bits(S), bits(V)) and out["n_thresholds"] > 0


def test_american_price_is_the_oracles_on_the_device_matrix_and_the_greeks_base(ctx):
    from options_model_amd import price_american_greeks, price_american_option
    from helpers import greeks_ref as gr
    from helpers.greeks_check import agrees as _agrees

    hp = qe.SET_B
    M, N = 20_004, 37
    V = paths(ctx, hp, M, N, seed=42, stream=0)
    for is_put in (True, False):
        ref = orc.lsm_poly(V, K, R, T, is_put, "two_pass")
        ot = "put" if is_put else "call"
        got = price_american_option(S0, K, R, None, T, M, N, model="Heston", option_type=ot, heston_params=hp,
                                    heston_scheme="qe", seed=42, stream=0, ctx=ctx)
        assert (got.n_exercised, got.sum_nitm) == (ref["n_exercised"], ref["sum_nitm"]), is_put
        assert abs(got.price - ref["price"]) <= 1e-9 * ref["price"]
        ffi = ctx.price_american(params(hp, M, N, is_put=is_put, seed=42, stream=0))
        assert ffi["price"] == got.price and ffi["n_zero"] == ref["n_zero"]
        g = price_american_greeks(S0, K, R, None, T, M, N, model="Heston", option_type=ot, heston_params=hp,
                                  heston_scheme="qe", seed=42, stream=0, ctx=ctx)
        assert abs(g.price - got.price) <= 1e-12 * got.price
        # the spot is linear in S0, so the pathwise delta and gamma of the frozen policy need nothing of the scheme: the
        # restatement of tests/helpers/greeks_ref.py on the device's QE matrix, at the bounds of tests/test_gpu_greeks.py
        pp = params(hp, M, N, is_put=is_put, seed=42, stream=0)
        d = ctx.price_american_greeks(pp, bump=0.01, want_betas=True)
        _agrees(d, gr.greeks(V, K, R, T, is_put, d["betas"], S0, 0.0, h=0.01, gbm=False), pp)
        assert (g.delta, g.gamma) == (d["delta"], d["gamma"]) and (g.delta < 0.0) == is_put
    # S0 scales every spot of the matrix exactly where the scale is a power of two: what the pathwise delta rests on
    V2 = paths(ctx, hp, M, N, seed=42, stream=0, s0=2.0 * S0)
    assert np.array_equal(bits(V2), bits(2.0 * V))


def test_batched_pricings_are_the_single_calls(ctx):
    hp = qe.SET_B
    ps = [params(hp, M, N, is_put=(i % 2 == 0), stream=4 + i) for i, (M, N) in enumerate([(514, 5), (4096, 9), (254, 4)])]
    for p, res in zip(ps, ctx.price_american_batch(ps)):
        one = ctx.price_american(p)
        assert res["n_exercised"] == one["n_exercised"] and abs(res["price"] - one["price"]) <= 1e-12 * abs(one["price"])


# ---------------------------------------------------------------------------------------------- 6. known answers
@pytest.fixture(scope="module")
def case_one(ctx):
    """Case I (T = 10, xi = 1, rho = -0.9) at 40 quarter-year steps on the stream of tests/test_heston_qe_cpu.py: the device's
    QE and full-truncation terminal spots"""
    c, N, M = qe.CASE_I, qe.BIAS_N, 2 * qe.BIAS_PAIRS
    hp = {k: c[k] for k in ("v0", "kappa", "theta", "xi", "rho")}
    kw = dict(seed=qe.BIAS_SEED, stream=qe.BIAS_STREAM, s0=c["S0"], r=c["r"], t=c["T"])
    return dict(qe=paths(ctx, hp, M, N, scheme=QE, **kw)[-1], ft=paths(ctx, hp, M, N, scheme=FT, **kw)[-1])


def test_case_one_price_and_what_full_truncation_gives(case_one):
    from test_heston_qe_cpu import bias_stats

    exact = qe.price(**qe.CASE_I)
    b = bias_stats(case_one["qe"], case_one["ft"])
    print(f"Case I, dt = 1/4, {2 * qe.BIAS_PAIRS} paths: exact {exact:.5f}; device QE {b['qe']:.5f} (se {b['se_qe']:.5f}), "
          f"full truncation {b['ft']:.5f} (se {b['se_ft']:.5f}); paired se {b['se_diff']:.5f}")
    assert abs(b["qe"] - (exact + qe.QE_OFFSET)) <= 4.0 * b["se_qe"], b
    assert abs(b["ft"] - exact) - abs(b["qe"] - exact) > 4.0 * b["se_diff"], b


def test_case_one_mean_terminal_spot_is_the_restatements(case_one):
    c, P = qe.CASE_I, qe.BIAS_PAIRS
    st = case_one["qe"].astype(np.float64) * math.exp(-c["r"] * c["T"])
    pair = 0.5 * (st[:P] + st[P:])
    print(f"mean discounted terminal spot {pair.mean():.6f} (se {pair.std() / math.sqrt(P):.6f}); restatement {qe.QE_MEAN_ST:.6f}")
    assert abs(pair.mean() - qe.QE_MEAN_ST * math.exp(-c["r"] * c["T"])) <= 4.0 * pair.std() / math.sqrt(P)


# ---------------------------------------------------------------------------------------------- 7. determinism, refusals
def test_two_calls_give_equal_bytes(ctx):
    for name, hp in qe.SETS.items():
        a, b = paths(ctx, hp, 2050, 33), paths(ctx, hp, 2050, 33)
        assert a.tobytes() == b.tobytes(), name
    p = params(qe.SET_B, 4096, 20)
    a, b = ctx.price_american(p), ctx.price_american(p)
    assert [a[k] for k in KEYS] == [b[k] for k in KEYS]


def test_refusals_launch_nothing(ctx):
    M, N = 64, 4
    S = ctx.to_device(np.full((N + 1, M), 7.0, np.float32))
    try:
        def rc(scheme, **over):
            hp = dict(qe.SET_A, **over)
            return ctx.lib.omc_heston_paths_f32(ctx.handle, S.ptr, M, M, N, S0, R, T, *hp_list(hp), qe.SEED, 0, 0, scheme)

        assert rc(QE, xi=0.0) == -36 and rc(QE, kappa=0.0) == -36 and rc(QE, xi=-0.1) == -36 and rc(QE, theta=0.0) == -36
        assert rc(4) == -4 and rc(-1) == -4
        assert rc(FT, xi=0.0) == 0  # the Euler schemes take it, as before
        S2 = ctx.to_device(np.full((N + 1, M), 7.0, np.float32))
        try:
            sv = lambda scheme, **over: ctx.lib.omc_heston_paths_sv_f32(  # noqa: E731
                ctx.handle, S2.ptr, S2.ptr, M, M, N, S0, R, T, *hp_list(dict(qe.SET_A, **over)), qe.SEED, 0, 0, scheme)
            assert sv(QE, kappa=0.0) == -36 and sv(4) == -4
            assert np.all(S2.to_host() == 7.0)  # nothing was written
        finally:
            S2.free()
        res = _ffi.Result()
        for over in (dict(xi=0.0), dict(kappa=0.0)):
            p = params(dict(qe.SET_A, **over), M, N)
            assert ctx.lib.omc_price_american(ctx.handle, C.byref(p), C.byref(res), None, 0) == -36
            assert ctx.lib.omc_price_european(ctx.handle, C.byref(p), C.byref(res)) == -36
        p4 = params(qe.SET_A, M, N, scheme=4)
        assert ctx.lib.omc_price_american(ctx.handle, C.byref(p4), C.byref(res), None, 0) == -4
        k = np.array([100.0])
        out = np.zeros(2)
        assert ctx.lib.omc_heston_price_strikes(ctx.handle, M, N, S0, R, T, 0.04, 2.0, 0.04, 0.0, -0.7, qe.SEED, 0, QE,
                                                k.ctypes.data, 1, 0, out.ctypes.data, out[1:].ctypes.data) == -36
    finally:
        S.free()
    # the price bounds keep refusing everything but schemes 0 and 1: scheme 3 does not reach a kernel as "the last one"
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.n_lower, cfg.n_outer, cfg.n_inner = 1, 1000, 64, 64
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    for reg in (0, 1):
        cfg.regressors = reg
        p = params(qe.SET_A, 4096, 8)
        assert ctx.lib.omc_price_american_bounds_heston(ctx.handle, C.byref(p), C.byref(cfg), None, None, None, None,
                                                        C.byref(out)) == -12
    # the context still prices
    assert ctx.price_american(params(qe.SET_A, 4096, 8))["price"] > 0.0


def test_c_example_prices_the_atm_put(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_heston_qe"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_heston_qe.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "50", "100000"], check=True, capture_output=True, text=True, timeout=300).stdout
    hp = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
    ref = ctx.price_american(params(hp, 100_000, 50, seed=42, stream=0))
    assert f"qe: price {ref['price']:.6f}" in out, out
    assert "xi = 0 under qe: -36" in out

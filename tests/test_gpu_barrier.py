"""Barrier options (omc_price_barrier, options_model_amd/csrc/omc_barrier.hip).

The encoded matrix against the encoder of tests/helpers/barrier_ref.py applied to the vanilla generator's matrix (bit for
bit), the continuous-monitoring hit steps against a numpy restatement on the documented Philox counters, the American
price against the C oracle's two-pass flow on the device's own matrix, the European sums against omc_price_european and
the closed forms, shards, refusals, the facade, the v2 compat class and the C example."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import barrier_ref as br
from oracle import cpu as orc
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

S0, K, R, SIG, T = 100.0, 100.0, 0.05, 0.2, 1.0
HES = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
MODELS = [("gbm", 0), ("heston", 0), ("heston", 1), ("heston", 2)]


def _H(kind, far=False):
    if kind.startswith("down"):
        return 1e-6 * S0 if far else 90.0
    return 1e6 * S0 if far else 112.0


def _params(model="gbm", scheme=0, is_put=True, M=4096, N=50, S0_=S0, K_=K, seed=42, stream=3, pair_offset=0, **kw):
    return _ffi.make_params(model=model, heston_scheme=scheme, is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N,
                            S0=S0_, K=K_, r=R, sigma=SIG, T=T, seed=seed, stream=stream, pair_offset=pair_offset,
                            **{**HES, **kw})


def _vanilla(ctx, p):
    if p.model == 1:
        S = ctx.heston_paths(p.n_paths, p.n_steps, p.S0, p.r, p.T, p.v0, p.kappa, p.theta, p.xi, p.rho, p.seed, p.stream,
                             p.pair_offset, scheme=p.heston_scheme)
    else:
        S = ctx.gbm_paths(p.n_paths, p.n_steps, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, p.pair_offset)
    out = S.to_host()
    S.free()
    return out


def _barrier(ctx, p, kind, H, monitoring="discrete", american=True):
    keep = ctx.empty((p.n_steps + 1, p.n_paths), np.float32)
    out = ctx.price_barrier(p, kind, H, monitoring=monitoring, american=american, keep_paths=keep)
    S = keep.to_host()
    keep.free()
    return out, S


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ 1. encoding
@pytest.mark.parametrize("N", [50, 51])
@pytest.mark.parametrize("model,scheme", MODELS)
def test_encoded_matrix_is_the_vanilla_matrix_encoded_bit_for_bit(ctx, model, scheme, N):
    for is_put in (True, False):
        p = _params(model, scheme, is_put=is_put, N=N)
        V = _vanilla(ctx, p)
        dead = br.dead_spot(K, is_put)
        for kind in br.KINDS:
            H = _H(kind)
            out, S = _barrier(ctx, p, kind, H)
            ref = br.encode(V, kind, H, K=K, is_put=is_put)
            assert np.array_equal(_bits(S), _bits(ref)), (model, scheme, N, is_put, kind)
            hs = br.discrete_hit_steps(V, kind, H)
            t = np.arange(N + 1)[:, None]
            live = (t >= hs[None, :]) if kind.endswith("-in") else (t < hs[None, :])
            assert np.array_equal(_bits(S[live]), _bits(V[live]))
            assert np.all(_bits(S[~live]) == _bits(np.float32(dead)))
            assert 0 < (~live).sum() < live.size  # the barrier is met by some paths, not all
            assert out["hit_prob"] == (hs <= N).mean()


# ------------------------------------------------------------------ 2. continuous monitoring
@pytest.mark.parametrize("N", [50, 51])
def test_continuous_hit_steps_match_the_restatement(ctx, N):
    M = 4096
    P = M // 2
    p = _params(N=N, seed=7, stream=5)
    V = _vanilla(ctx, p)
    Z = orc.gbm_normals(P, N, 7, 5)
    u = br.bridge_uniforms(P, N, 7, 5)
    ties = 0
    for kind in br.KINDS:
        H = _H(kind)
        out, S = _barrier(ctx, p, kind, H, monitoring="continuous")
        hs_ref, gap = br.continuous_hit_steps(V, Z, u, S0, H, R, SIG, T, kind)
        ref = br.encode(V, kind, H, hit_steps=hs_ref, K=K, is_put=True)
        bad = np.nonzero(np.any(_bits(S) != _bits(ref), axis=0))[0]
        for j in bad:  # a disagreement only where the bridge test is a tie
            assert gap[:, j].min() <= 1e-6, (kind, j)
        ties += len(bad)
        t = np.arange(N + 1)[:, None]
        hs_dis = br.discrete_hit_steps(V, kind, H)
        assert np.all(hs_ref <= hs_dis)  # continuous monitoring hits no later than discrete
        live_ref = (t >= hs_ref[None, :]) if kind.endswith("-in") else (t < hs_ref[None, :])
        ok = np.ones(M, bool)
        ok[bad] = False
        assert np.array_equal(_bits(S[:, ok][live_ref[:, ok]]), _bits(V[:, ok][live_ref[:, ok]]))
        assert (hs_ref < hs_dis).sum() > 0  # the bridge adds hits between grid points
    assert ties <= 2, ties


# ------------------------------------------------------------------ 3. American against the C oracle
def _check_american(ctx, p, kind, H, monitoring="discrete"):
    out, S = _barrier(ctx, p, kind, H, monitoring=monitoring)
    ref = orc.lsm_poly(S, p.K, p.r, p.T, bool(p.is_put), "two_pass")
    assert (out["n_exercised"], out["n_zero"]) == (ref["n_exercised"], ref["n_zero"]), (kind, out, ref)
    assert abs(out["price"] - ref["price"]) <= 1e-9 * max(ref["price"], 1e-12), (kind, out["price"], ref["price"])
    assert out["folded"] == 0
    return out


@pytest.mark.parametrize("monitoring", ["discrete", "continuous"])
@pytest.mark.parametrize("is_put", [True, False])
def test_american_matches_the_oracle_on_the_encoded_matrix_gbm(ctx, monitoring, is_put):
    p = _params(is_put=is_put, M=16384, N=50, stream=11)
    for kind in br.KINDS:
        out = _check_american(ctx, p, kind, _H(kind), monitoring)
        assert out["price"] > 0.0


@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_american_matches_the_oracle_on_the_encoded_matrix_heston(ctx, scheme):
    for is_put in (True, False):
        p = _params("heston", scheme, is_put=is_put, M=16384, N=40, stream=12)
        for kind in br.KINDS:
            _check_american(ctx, p, kind, _H(kind))


def test_american_random_sweep_against_the_oracle(ctx):
    rng = np.random.default_rng(2024)
    for i in range(20):
        kind = br.KINDS[rng.integers(4)]
        s0 = float(rng.uniform(80, 120))
        H = s0 * (float(rng.uniform(0.7, 0.97)) if kind.startswith("down") else float(rng.uniform(1.03, 1.3)))
        k_ = s0 * float(rng.uniform(0.85, 1.15))
        N = int(rng.integers(2, 80))
        M = 2 * int(rng.integers(500, 6000))
        model, scheme = MODELS[rng.integers(4)]
        mon = "continuous" if model == "gbm" and rng.random() < 0.4 else "discrete"
        p = _params(model, scheme, is_put=bool(rng.integers(2)), M=M, N=N, S0_=s0, K_=k_, seed=100 + i, stream=i)
        _check_american(ctx, p, kind, H, mon)


# ------------------------------------------------------------------ 4. far barriers
@pytest.mark.parametrize("model,scheme", [("gbm", 0), ("heston", 1)])
def test_far_barrier_is_the_vanilla_full_storage_pricing(ctx, model, scheme):
    p = _params(model, scheme, M=65536, N=50, stream=21)
    ctx.set_option("fold_antithetic", 0)
    try:
        van = ctx.price_american(p)
    finally:
        ctx.set_option("fold_antithetic", 1)
    ko = ctx.price_barrier(p, "down-and-out", 1e-6 * S0)
    assert (ko["price"], ko["sumsq"], ko["n_exercised"], ko["n_zero"], ko["sum_nitm"]) == \
        (van["price"], van["sumsq"], van["n_exercised"], van["n_zero"], van["sum_nitm"])
    assert ko["hit_prob"] == 0.0 and ko["folded"] == 0
    ki = ctx.price_barrier(p, "down-and-in", 1e-6 * S0)
    assert ki["price"] == 0.0 and ki["n_exercised"] == 0 and ki["hit_prob"] == 0.0


# ------------------------------------------------------------------ 5. European
@pytest.mark.parametrize("model,scheme", MODELS)
def test_european_sums_without_the_matrix_equal_those_of_the_american_call(ctx, model, scheme):
    keys = ("euro_out", "euro_out_se", "euro_in", "euro_in_se", "hit_prob")
    for kind in ("down-and-out", "up-and-in"):
        p = _params(model, scheme, M=100000, N=50, stream=31)
        eu = ctx.price_barrier(p, kind, _H(kind), american=False)
        am = ctx.price_barrier(p, kind, _H(kind), american=True)
        assert tuple(eu[k] for k in keys) == tuple(am[k] for k in keys)
        van = ctx.price_european(p)
        assert abs(eu["euro_in"] + eu["euro_out"] - van["price"]) <= 1e-12 * van["price"]
        assert 0.0 < eu["hit_prob"] < 1.0
        base = eu["euro_in"] if kind.endswith("-in") else eu["euro_out"]
        assert eu["price"] == base


@pytest.mark.parametrize("kind", br.KINDS)
@pytest.mark.parametrize("is_put", [True, False])
def test_continuous_european_matches_the_closed_form(ctx, kind, is_put):
    H = 85.0 if kind.startswith("down") else 120.0
    p = _params(is_put=is_put, M=4_000_000, N=50, stream=41)
    eu = ctx.price_barrier(p, kind, H, monitoring="continuous", american=False)
    ref = br.closed_form(kind, is_put, S0, K, H, R, SIG, T)
    v, se = (eu["euro_in"], eu["euro_in_se"]) if kind.endswith("-in") else (eu["euro_out"], eu["euro_out_se"])
    assert abs(v - ref) <= 4 * se + 1e-9, (v, se, ref)


def test_american_knock_out_is_worth_at_least_the_european(ctx):
    for is_put, kind in ((True, "down-and-out"), (False, "up-and-out"), (True, "up-and-out")):
        p = _params(is_put=is_put, M=262144, N=50, stream=51)
        am = ctx.price_barrier(p, kind, _H(kind))
        assert am["price"] >= am["euro_out"] - 3 * am["euro_out_se"], (kind, am)


# ------------------------------------------------------------------ 6. shards
@pytest.mark.parametrize("model,scheme,monitoring", [("gbm", 0, "discrete"), ("gbm", 0, "continuous"),
                                                      ("heston", 2, "discrete")])
def test_two_pair_offset_shards_are_the_whole_run(ctx, model, scheme, monitoring):
    M, N = 4096, 33
    P, Ps = M // 2, M // 4
    _, whole = _barrier(ctx, _params(model, scheme, M=M, N=N, stream=61), "up-and-out", 112.0, monitoring)
    for k in range(2):
        _, sh = _barrier(ctx, _params(model, scheme, M=M // 2, N=N, stream=61, pair_offset=k * Ps), "up-and-out", 112.0,
                         monitoring)
        assert np.array_equal(_bits(sh[:, :Ps]), _bits(whole[:, k * Ps:(k + 1) * Ps]))
        assert np.array_equal(_bits(sh[:, Ps:]), _bits(whole[:, P + k * Ps:P + (k + 1) * Ps]))


# ------------------------------------------------------------------ 7. refusals
def _rc(ctx, p, kind=0, monitoring=0, american=1, H=90.0):
    b = _ffi.Barrier()
    b.kind, b.monitoring, b.american, b.H = kind, monitoring, american, H
    out = _ffi.BarrierResult()
    return ctx.lib.omc_price_barrier(ctx.handle, C.byref(p), C.byref(b), C.byref(out), None, 0)


def test_refusals_have_their_own_codes_and_leave_the_context_usable(ctx):
    p = _params(M=4096, N=20)
    ref = ctx.price_barrier(p, "down-and-out", 90.0)
    per_step = _params(M=4096, N=20)
    per_step.semantics = 0
    assert _rc(ctx, per_step) == -11
    assert _rc(ctx, per_step, american=0) == 0  # the European needs no flow
    assert _rc(ctx, _params("heston", 0, M=4096, N=20), monitoring=1) == -12
    for H in (0.0, -5.0, float("nan"), float("inf")):
        assert _rc(ctx, p, H=H) == -13
    assert _rc(ctx, p, kind=0, H=100.0) == -14  # S0 on the barrier
    assert _rc(ctx, p, kind=2, H=120.0) == -14  # down barrier above S0
    assert _rc(ctx, p, kind=1, H=95.0) == -14   # up barrier below S0
    assert _rc(ctx, p, kind=4) == -15 and _rc(ctx, p, monitoring=2) == -15 and _rc(ctx, p, american=2) == -15
    non_anti = _params(M=4096, N=20)
    non_anti.antithetic = 0
    assert _rc(ctx, non_anti) == -15
    bad = _params(M=4096, N=20)
    bad.n_paths = 0
    assert _rc(ctx, bad) == -3
    with pytest.raises(ValueError, match="S0 lies on or beyond"):
        ctx.price_barrier(p, "down-and-out", 100.0)
    again = ctx.price_barrier(p, "down-and-out", 90.0)
    assert (again["price"], again["n_exercised"], again["euro_out"]) == (ref["price"], ref["n_exercised"], ref["euro_out"])


def test_distributed_context_is_refused(ctx):
    c = _ffi.Context(0)
    try:
        c.set_allreduce_hook(lambda dptr, count: None)
        assert _rc(c, _params(M=4096, N=20)) == -10
        c.set_allreduce_hook(None)
        assert _rc(c, _params(M=4096, N=20)) == 0
    finally:
        c.close()


# ------------------------------------------------------------------ 8. facade, compat, C example
def test_facade_and_compat_agree_with_the_binding(ctx):
    from options_model_amd import BarrierResult, price_barrier_option
    from options_model_amd.compat.options_model_2 import ExoticOptionPricer
    kw = dict(S0=S0, K=K, r=R, sigma=SIG, T=T, n_paths=20000, n_steps=50, barrier=90.0, barrier_type="down-and-out",
              option_type="put", seed=42, stream=9)
    f = price_barrier_option(ctx=ctx, **kw)
    assert isinstance(f, BarrierResult)
    d = ctx.price_barrier(_params(M=20000, N=50, seed=42, stream=9), "down-and-out", 90.0)
    assert (f.price, f.n_exercised, f.hit_prob, f.euro_out, f.euro_in) == \
        (d["price"], d["n_exercised"], d["hit_prob"], d["euro_out"], d["euro_in"])
    assert f.stderr > 0 and f.timings_ms["barrier_paths"] > 0
    assert ExoticOptionPricer.price_barrier_option(ctx=ctx, **kw) == d["price"]
    fe = price_barrier_option(ctx=ctx, style="european", monitoring="continuous", **{**kw, "barrier_type": "down-and-in"})
    de = ctx.price_barrier(_params(M=20000, N=50, seed=42, stream=9), "down-and-in", 90.0, monitoring="continuous",
                           american=False)
    assert fe.price == de["euro_in"] and fe.n_exercised == 0
    fh = price_barrier_option(ctx=ctx, model="Heston", heston_scheme="full_truncation", **{**kw, "option_type": "call",
                                                                                           "barrier_type": "up-and-out",
                                                                                           "barrier": 115.0})
    dh = ctx.price_barrier(_params("heston", 1, is_put=False, M=20000, N=50, seed=42, stream=9), "up-and-out", 115.0)
    assert fh.price == dh["price"]


def test_c_host_example_prints_the_binding_numbers(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "barrier"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "barrier.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "200000", "50"], check=True, capture_output=True, text=True, timeout=300).stdout
    p_put = _ffi.make_params(semantics="two_pass", n_paths=200000, n_steps=50, seed=42)
    ref1 = ctx.price_barrier(p_put, "down-and-out", 90.0)
    p_call = _ffi.make_params(semantics="two_pass", is_put=False, n_paths=200000, n_steps=50, seed=42)
    ref2 = ctx.price_barrier(p_call, "up-and-in", 120.0, monitoring="continuous", american=False)
    for name, ref in (("down-and-out american put", ref1), ("up-and-in european call", ref2)):
        line = re.search(rf"^{name}: price ([-0-9.]+)  exercised (\d+)  hit_prob ([-0-9.]+)", out, flags=re.M)
        assert line, out
        assert abs(float(line.group(1)) - ref["price"]) < 1e-6
        assert int(line.group(2)) == ref["n_exercised"]
        assert abs(float(line.group(3)) - ref["hit_prob"]) < 1e-6
        eu = re.search(rf"^{name}: euro_out ([-0-9.]+) se [-0-9.]+  euro_in ([-0-9.]+)", out, flags=re.M)
        assert abs(float(eu.group(1)) - ref["euro_out"]) < 1e-6 and abs(float(eu.group(2)) - ref["euro_in"]) < 1e-6

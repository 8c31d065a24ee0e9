"""Andersen-Broadie price bounds (omc_price_american_bounds, options_model_amd/csrc/omc_bounds.hip).

The device's Q^_t, samples, bounds and counts against the numpy restatement of tests/helpers/bounds_ref.py on the
device's own spots (the generators at the documented streams and pair offsets; sweep 14 of tests/test_gpu_fuzz.py runs
the same comparison over random shapes), a call of three inner launches restated on sampled outer paths, the bracket around
the Bermudan lattice,
known answers at one exercise date and for a never-exercising policy, determinism, refusals, the facade and the C
example."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_ref as br
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
POLICIES = ["textbook", "two_pass", "reference", "given"]


def _params(is_put=True, S0=100.0, N=8, M=4096, stream=0, model="gbm"):
    return _ffi.make_params(model=model, is_put=is_put, semantics="two_pass", n_paths=M, n_steps=N, S0=S0, K=K, r=R,
                            sigma=SIG, T=T, seed=42, stream=stream)


def _given_table(ctx, N, is_put):
    """a policy from other paths (stream 9), textbook fits"""
    d = ctx.lsm_poly(ctx.gbm_paths(4096, N, 100.0, R, SIG, T, 42, 9), K, R, T, is_put, "textbook")
    b = np.zeros((N + 1, 4))
    b[:, :3], b[:, 3] = d["betas"], d["nitm"]
    return b


@pytest.fixture(scope="module")
def tiny(ctx):
    """The spots of the tiny case, from the device's generators at the documented streams / offsets."""
    N, n_outer, n_inner, n_lower = 8, 64, 64, 4096
    So = ctx.gbm_paths(n_outer, N, 100.0, R, SIG, T, 42, 2).to_host()
    Sl = ctx.gbm_paths(n_lower, N, 100.0, R, SIG, T, 42, 1).to_host()
    Zd = ctx.gbm_normals(n_outer * (N + 1) * n_inner // 2, N, 42, 3)
    Z = Zd.to_host()
    Zd.free()

    def spots(z, s0):
        S = ctx.gbm_paths_from_normals(z, s0, R, SIG, T)
        h = S.to_host()
        S.free()
        return h

    inner = br.inner_from_normals(Z, So, n_inner, spots)
    cache = {(i, t): inner(i, t) for i in range(n_outer) for t in range(N)}
    return dict(N=N, n_outer=n_outer, n_inner=n_inner, n_lower=n_lower, So=So, Sl=Sl, inner=lambda i, t: cache[(i, t)])


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("policy", POLICIES)
def test_device_equals_restatement(ctx, tiny, is_put, policy):
    N = tiny["N"]
    p = _params(is_put=is_put, N=N)
    given = _given_table(ctx, N, is_put) if policy == "given" else None
    d = ctx.price_american_bounds(p, policy=policy, n_lower=tiny["n_lower"], n_outer=tiny["n_outer"],
                                  n_inner=tiny["n_inner"], betas=given, want_q=True, want_samples=True)
    b4 = d["betas"]
    if policy == "given":
        np.testing.assert_array_equal(b4, given)
    else:  # omc_lsm_poly's fits on the paths of p
        ref = ctx.lsm_poly(ctx.gbm_paths(p.n_paths, N, 100.0, R, SIG, T, 42, 0), K, R, T, is_put, policy)
        np.testing.assert_array_equal(b4[:, :3], ref["betas"])
        np.testing.assert_array_equal(b4[:, 3], ref["nitm"])
    lo = br.lower_bound(tiny["Sl"], K, R, T, is_put, b4)
    up = br.upper_bound(tiny["So"], tiny["inner"], K, R, T, is_put, b4)
    assert lo["ties"] == 0 and up["ties"] == 0  # numpy's decisions are the device's
    assert d["n_exercised_lower"] == lo["n_exercised"]
    assert d["inner_path_steps"] == up["inner_path_steps"]
    np.testing.assert_allclose(d["q"], up["q"], rtol=1e-12, atol=1e-12 * K)
    np.testing.assert_allclose(d["samples"], up["samples"], rtol=1e-12, atol=1e-12 * K)
    for k in ("lower", "se_lower"):
        assert d[k] == pytest.approx(lo[k], rel=1e-12, abs=1e-12 * K), k
    for k in ("upper", "se_upper"):
        assert d[k] == pytest.approx(up[k], rel=1e-12, abs=1e-12 * K), k
    assert d["ci_lo"] == d["lower"] - 1.96 * d["se_lower"] and d["ci_hi"] == d["upper"] + 1.96 * d["se_upper"]
    assert (d["n_lower"], d["n_outer"], d["n_inner"]) == (tiny["n_lower"], tiny["n_outer"], tiny["n_inner"])


# GPU sizes of a few seconds; the put's gap threshold (2 % of V) comes from the CPU restatement
# (test_bounds_ref_cpu.py::test_tightness_threshold_from_restatement), not from these runs.
BIG = dict(n_lower=400_000, n_outer=4096, n_inner=512)


@pytest.mark.parametrize("S0,is_put", [(90.0, True), (100.0, True), (110.0, True), (100.0, False)])
def test_brackets_the_bermudan_value(ctx, S0, is_put):
    N = 50
    d = ctx.price_american_bounds(_params(is_put=is_put, S0=S0, N=N, M=100_000), policy="textbook", **BIG)
    V = br.lattice(S0, K, R, SIG, T, N, is_put=is_put)
    assert d["lower"] - 3 * d["se_lower"] <= V <= d["upper"] + 3 * d["se_upper"], (d, V)
    if is_put:
        assert 0.0 < d["upper"] - d["lower"] < 0.02 * V, (d, V)
    else:  # no dividends: the Bermudan call is the European
        bs = br.black_scholes(S0, K, R, SIG, T, False)
        assert d["lower"] - 3 * d["se_lower"] <= bs <= d["upper"] + 3 * d["se_upper"], (d, bs)


def test_launch_blocks_restated_on_sampled_outer_paths(ctx):
    """The inner kernel runs as launches over blocks of outer paths, each at most 2^30 worst-case inner steps
    (n_inner N (N+1) / 2 per outer path): at the sizes of the bracket test above that is blocks of 1644
    outer paths, three launches.  Q^ of the first, last and a middle outer path of every block, and of the antithetic
    partner columns of two of them, all 50 dates each, against the restatement on the device's own spots: q at rtol 1e-12
    (a mean of 512 summands >= 0 in either order), the samples at bounds_ref.samples_atol (the walk adds 2 t such values)."""
    N, n_outer, n_inner = 50, BIG["n_outer"], BIG["n_inner"]
    blk = (1 << 30) // (n_inner // 2 * N * (N + 1))
    starts = list(range(0, n_outer, blk))
    assert blk == 1644 and len(starts) >= 3  # a changed launch rule must not empty this test
    rows = []
    for i0 in starts:
        i1 = min(i0 + blk, n_outer)
        rows += [i0, (i0 + i1) // 2, i1 - 1]
    rows += [rows[1] + n_outer // 2, rows[2] + n_outer // 2]  # partner columns: other blocks' interiors
    assert len(set(rows)) == len(rows) and max(rows) < n_outer
    p = _params(N=N, M=20_000)
    d = ctx.price_american_bounds(p, policy="textbook", n_lower=4096, n_outer=n_outer, n_inner=n_inner, want_q=True,
                                  want_samples=True)

    def host(a):
        h = a.to_host()
        a.free()
        return h

    So = host(ctx.gbm_paths(n_outer, N, 100.0, R, SIG, T, 42, 2))
    inner = br.inner_by_item(lambda off, n: host(ctx.gbm_normals(n, N, 42, 3, off)), So, n_inner,
                             lambda z, s0: host(ctx.gbm_paths_from_normals(z, s0, R, SIG, T)))
    qr = br.q_rows(So, inner, rows, K, R, T, True, d["betas"])
    wk = br.walk_rows(So, qr["q"], rows, K, R, T, True, d["betas"])
    print(f"blocks of {blk}: rows {rows}, ties {qr['ties']} + {wk['ties']}")
    assert qr["ties"] == 0 and wk["ties"] == 0  # numpy's decisions are the device's
    np.testing.assert_allclose(d["q"][rows], qr["q"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(d["samples"][rows], wk["samples"], rtol=0, atol=br.samples_atol(N, qr["q"], wk["zmax"]))


@pytest.mark.parametrize("is_put", [True, False])
def test_one_date_is_black_scholes(ctx, is_put):
    d = ctx.price_american_bounds(_params(is_put=is_put, N=1, M=4096), **BIG)
    bs = br.black_scholes(100.0, K, R, SIG, T, is_put)
    assert abs(d["lower"] - bs) <= 4 * d["se_lower"], (d, bs)
    assert abs(d["upper"] - bs) <= 4 * d["se_upper"], (d, bs)
    assert d["n_exercised_lower"] == 0
    assert d["inner_path_steps"] == BIG["n_outer"] * BIG["n_inner"]


def test_never_exercise_table_gives_the_european(ctx):
    N = 50
    d = ctx.price_american_bounds(_params(N=N), policy="given", betas=np.zeros((N + 1, 4)), **BIG)
    bs = br.black_scholes(100.0, K, R, SIG, T, True)
    assert abs(d["lower"] - bs) <= 4 * d["se_lower"], (d, bs)
    assert d["n_exercised_lower"] == 0
    assert d["upper"] >= d["lower"] and d["upper"] + 3 * d["se_upper"] >= bs
    assert d["inner_path_steps"] == BIG["n_outer"] * BIG["n_inner"] * N * (N + 1) // 2


def test_deterministic_and_table_fallback(ctx):
    p = _params(N=50, M=20_000)
    kw = dict(n_lower=100_000, n_outer=2048, n_inner=256, want_q=True, want_samples=True)
    a = ctx.price_american_bounds(p, **kw)
    b = ctx.price_american_bounds(p, **kw)
    # every other step decided by the float64 rule instead of the tables: the same decisions, the same bits
    ctx.set_option("pass2_tables_irregular_every", 2)
    try:
        c = ctx.price_american_bounds(p, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    for x in (b, c):
        for k in ("lower", "se_lower", "upper", "se_upper", "n_exercised_lower", "inner_path_steps"):
            assert x[k] == a[k], k
        np.testing.assert_array_equal(x["q"], a["q"])
        np.testing.assert_array_equal(x["samples"], a["samples"])
        np.testing.assert_array_equal(x["betas"], a["betas"])


def _rc(ctx, p, policy=1, n_lower=1000, n_outer=64, n_inner=64, betas=None):
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    b = None if betas is None else np.ascontiguousarray(betas, np.float64)
    return ctx.lib.omc_price_american_bounds(ctx.handle, C.byref(p), C.byref(cfg), b.ctypes.data if b is not None else None,
                                             None, None, None, C.byref(out))


def test_refusals(ctx):
    p = _params()
    assert _rc(ctx, _params(model="heston")) == -12
    assert _rc(ctx, p, n_inner=63) == -3
    assert _rc(ctx, p, n_outer=63) == -3
    assert _rc(ctx, p, n_lower=999) == -3
    assert _rc(ctx, p, policy=7) == -4
    assert _rc(ctx, p, policy=3) == -7  # given without a table
    assert _rc(ctx, _params(N=252), n_outer=1 << 14, n_inner=1 << 12) == -16
    with pytest.raises(ValueError):
        ctx.price_american_bounds(p, policy="given", betas=np.zeros((5, 4)), n_lower=1000, n_outer=64, n_inner=64)
    with pytest.raises(ValueError):
        ctx.price_american_bounds(p, policy="lattice")
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _rc(hooked, p) == -10
    finally:
        hooked.close()


def test_facade_equals_ffi(ctx):
    from options_model_amd import price_american_bounds

    kw = dict(n_lower=100_000, n_outer=1024, n_inner=256)
    f = price_american_bounds(100.0, K, R, SIG, T, 20_000, 50, seed=42, stream=5, ctx=ctx, **kw)
    d = ctx.price_american_bounds(_params(N=50, M=20_000, stream=5), **kw)
    assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                              d["se_upper"], d["inner_path_steps"])
    np.testing.assert_array_equal(f.betas, d["betas"])
    assert f.policy == "textbook" and set(f.timings_ms) == {"fit", "lower", "upper", "total"}
    with pytest.raises(ValueError):
        price_american_bounds(100.0, K, R, SIG, T, 20_000, 50, n_inner=255, ctx=ctx)


def test_c_example_prints_the_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "50", "200000", "2048", "256"], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    ref = ctx.price_american_bounds(_params(N=50, M=100_000), n_lower=200_000, n_outer=2048, n_inner=256)
    lo, up = (float(v) for v in re.search(r"bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
    assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
    assert re.search(r"inner path-steps \d+", out) and "kernels:" in out
    assert not math.isnan(lo)

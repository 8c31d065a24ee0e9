"""Keys and counters of every entry point that draws ("the counter domains").

The Philox key is the 64-bit seed, split into (lo, hi) at a dozen places of the library; the counter is (pair lo, pair hi,
block or tagged block, stream low 32 bits).  The other tests use seeds below 2^32, single-digit streams and launches whose
pairs do not cross 2^32, so an entry point that dropped a key half or mishandled the carry would pass them.  Here every
drawing family of the call catalogue (tests/helpers/rng_keys.py; size class S) runs at seed 0x9E3779B97F4A7C15, stream
0xDEADBEEF, pair_offset 2^32 - 3:

  * the result differs when the seed's high half, its low half or stream bit 31 is cleared, and at pair_offset + 1 and + 2^32
  * the result is bit-identical at stream + 2^32 (include/omc.h: only the low 32 bits are used)
  * across the carry: a call with 8 pairs at 2^32 - 3 has, column by column, the bits of single-pair calls at 2^32 - 3 + j
  * the generators match the C oracle there at the contract's tolerances, and every family that keeps its matrix keeps
    the bits its own test file compares it to
  * the four price-bound families, whose lower, outer and inner simulations each split the key on their own (a result that
    merely changes with the seed proves nothing about each of them), equal their restatements on the device's own spots
"""
import numpy as np
import pytest

import test_gpu_barrier as tb
import test_gpu_basket as tk
import test_gpu_dividends as td
import test_gpu_generator_widths as tw
import test_gpu_jumps as tj
from helpers import barrier_ref as br
from helpers import basket_bounds_case as bc
from helpers import bounds_ref
from helpers import call_catalogue as cat
from helpers import dividend_ref as dr
from helpers import heston_bounds_case as hc
from helpers import jump_ref as jr
from helpers import runnerup_ref as rr
from helpers import rng_keys as rk
from helpers.heston_qe_ref import SET_B
from oracle import cpu as orc
from options_model_amd import _ffi
from test_gpu_dividends import bits

pytestmark = pytest.mark.gpu

SEED, STREAM, OFF = rk.BASE
HP = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
_base = {}


def base(ctx, name):
    """the entry at the base triple: computed once, shared"""
    if name not in _base:
        _base[name] = cat.run_at(name, ctx, *rk.BASE)
    return _base[name]


def host(a):
    h = a.to_host()
    a.free()
    return h


# ------------------------------------------------------------------ 1. every key half and counter word matters
@pytest.mark.parametrize("name", rk.entries())
def test_every_key_half_and_counter_word_changes_the_result(ctx, name):
    ref = base(ctx, name)
    assert ref and not cat.diff(ref, cat.run_at(name, ctx, *rk.BASE)), name  # (and the call repeats)
    for what, triple in rk.changes(cat.BY_NAME[name].family).items():
        assert cat.diff(ref, cat.run_at(name, ctx, *triple)), f"{name}: same result with the {what}"


@pytest.mark.parametrize("name", [n for n in rk.entries() if "stream" in rk.DRAWING[cat.BY_NAME[n].family]])
def test_only_the_streams_low_32_bits_are_used(ctx, name):
    assert cat.diff(base(ctx, name), cat.run_at(name, ctx, SEED, STREAM + (1 << 32), OFF)) == []


# ------------------------------------------------------------------ 2. across the carry of the pair counter
N9 = tw.N


def _generators():
    def normals(ctx, M, off):
        return [host(ctx.gbm_normals(M // 2, N9, SEED, STREAM, off))]

    def gbm(ctx, M, off):
        return [host(ctx.gbm_paths(M, N9, 100.0, 0.05, 0.2, 1.0, SEED, STREAM, off))]

    def heston(scheme):
        def run(ctx, M, off):
            law = SET_B if scheme == 3 else HP
            return [host(ctx.heston_paths(M, N9, 100.0, 0.05, 1.0, seed=SEED, stream=STREAM, pair_offset=off, scheme=scheme, **law))]
        return run

    def heston_sv(ctx, M, off):
        S, V = ctx.heston_paths_sv(M, N9, 100.0, 0.05, 1.0, seed=SEED, stream=STREAM, pair_offset=off, scheme=1, **HP)
        return [host(S), host(V)]

    out = {"gbm_normals": normals, "gbm_paths": gbm, "heston_paths_sv": heston_sv}
    out.update({f"heston_paths{s}": heston(s) for s in (0, 1, 2, 3)})
    return out


def _fused(call, model="gbm", scheme=0, d=0, **law):
    def run(ctx, M, off):
        p = td.params(model, scheme, M=M, N=N9, seed=SEED, stream=STREAM, pair_offset=off, **law)
        keep = ctx.to_device(np.full((N9 + 1, M), tw.SENTINEL, np.float32))
        akeep = ctx.to_device(np.full((d, N9 + 1, M), tw.SENTINEL, np.float32)) if d else None
        try:
            call(ctx, p, keep, akeep)
            return [a.to_host() for a in (keep, akeep) if a is not None]
        finally:
            keep.free()
            if akeep is not None:
                akeep.free()
    return run


def _american(ctx, p, keep, akeep):
    return ctx.price_american(p, keep_paths=keep)


def _continuous_barrier(ctx, p, keep, akeep):
    return ctx.price_barrier(p, "down-and-out", 90.0, monitoring="continuous", american=True, keep_paths=keep)


CARRY = dict(_generators(), **{
    "price_american": _fused(_american), "price_american-heston3": _fused(_american, "heston", 3, **SET_B),
    "price_barrier": _fused(tw._barrier), "price_barrier-continuous": _fused(_continuous_barrier),
    "price_american_div": _fused(tw._dividends), "price_american_div-heston2": _fused(tw._dividends, "heston", 2),
    "price_american_jump": _fused(tw._jumps), "price_american_jump-heston0": _fused(tw._jumps, "heston", 0),
    "price_american_basket": _fused(tw._basket, d=2)})


@pytest.mark.parametrize("name", list(CARRY))
def test_eight_pairs_across_the_carry_are_eight_single_pair_calls(ctx, name):
    run = CARRY[name]
    big = run(ctx, 16, OFF)
    for a in big:
        assert np.isfinite(a).all() and (a != tw.SENTINEL).all(), name
    for j in range(8):
        one = run(ctx, 2, OFF + j)
        for a, b in zip(big, one):
            if name == "gbm_normals":
                assert np.array_equal(bits(a[:, j]), bits(b[:, 0])), (name, j)
            else:
                assert np.array_equal(bits(a[..., j]), bits(b[..., 0])) and np.array_equal(bits(a[..., j + 8]), bits(b[..., 1])), (name, j)
    cols = [big[0][..., j] for j in range(8)]
    assert all(not np.array_equal(bits(cols[i]), bits(cols[i + 1])) for i in range(7)), name  # eight different pairs


# ------------------------------------------------------------------ 3. the generators against the oracle at the base triple
M3, N3 = 2002, 13  # 1,001 pairs (one pair per thread, more than one workgroup); the carry falls on the fourth pair


def test_generators_match_the_oracle_at_the_base_triple(ctx):
    Z = host(ctx.gbm_normals(M3 // 2, N3, SEED, STREAM, OFF))
    assert np.abs(Z - orc.gbm_normals(M3 // 2, N3, SEED, STREAM, OFF)).max() <= 4e-6
    S = host(ctx.gbm_paths(M3, N3, 100.0, 0.05, 0.2, 1.0, SEED, STREAM, OFF))
    assert np.abs(S / orc.gbm_paths(M3, N3, 100.0, 0.05, 0.2, 1.0, SEED, STREAM, OFF) - 1).max() <= 2e-5
    for scheme in (0, 1, 2):
        S = host(ctx.heston_paths(M3, N3, 100.0, 0.05, 1.0, seed=SEED, stream=STREAM, pair_offset=OFF, scheme=scheme, **HP))
        So = orc.heston_paths(M3, N3, 100.0, 0.05, 1.0, seed=SEED, stream=STREAM, pair_offset=OFF, scheme=scheme, **HP)
        assert np.abs(S / So - 1).max() <= 5e-5, scheme
    # another key half, stream bit or pair word is another sample altogether
    for seed, stream, off in rk.changes("gbm_normals").values():
        assert np.abs(Z - orc.gbm_normals(M3 // 2, N3, seed, stream, off)).max() > 1.0


# ------------------------------------------------------------------ 4. the kept matrices at the base triple
def test_price_american_keeps_the_generators_matrix(ctx):
    for model, scheme in td.MODELS:
        p = td.params(model, scheme, M=M3, N=N3, seed=SEED, stream=STREAM, pair_offset=OFF)
        keep = ctx.empty((N3 + 1, M3), np.float32)
        out = ctx.price_american(p, keep_paths=keep)
        S = host(keep)
        assert np.array_equal(bits(S), bits(td.vanilla(ctx, p, 0.0))), (model, scheme)
        td.check_price(out, S, p)


def test_barrier_keeps_the_encoded_vanilla_matrix(ctx):
    p = tb._params(M=M3, N=N3, seed=SEED, stream=STREAM, pair_offset=OFF)
    V = tb._vanilla(ctx, p)
    Z = orc.gbm_normals(M3 // 2, N3, SEED, STREAM, OFF)
    u = br.bridge_uniforms(M3 // 2, N3, SEED, STREAM, OFF)
    ties = 0
    for kind in br.KINDS:
        H = tb._H(kind)
        _, S = tb._barrier(ctx, p, kind, H)
        assert np.array_equal(bits(S), bits(br.encode(V, kind, H, K=tb.K, is_put=True))), kind
        _, S = tb._barrier(ctx, p, kind, H, monitoring="continuous")
        hs, gap = br.continuous_hit_steps(V, Z, u, tb.S0, H, tb.R, tb.SIG, tb.T, kind)
        ref = br.encode(V, kind, H, hit_steps=hs, K=tb.K, is_put=True)
        bad = np.nonzero(np.any(bits(S) != bits(ref), axis=0))[0]
        for j in bad:  # tests/test_gpu_barrier.py: a disagreement only where the bridge test is a tie
            assert gap[:, j].min() <= 1e-6, (kind, j)
        ties += len(bad)
        assert (hs < br.discrete_hit_steps(V, kind, H)).sum() > 0  # the bridge uniforms are in play
    assert ties <= 2, ties


@pytest.mark.parametrize("model,scheme", td.MODELS)
def test_dividends_keep_the_restated_matrix(ctx, model, scheme):
    p = td.params(model, scheme, M=M3, N=N3, seed=SEED, stream=STREAM, pair_offset=OFF)
    divs, _ = td.mixed_schedule(p, model)
    out, S = td.priced(ctx, p, 0.01, divs)
    td.check_matrix(ctx, p, 0.01, divs, S, model)
    td.check_price(out, S, p)


@pytest.mark.parametrize("model,scheme", td.MODELS)
def test_jumps_keep_the_restated_matrix(ctx, model, scheme):
    p = td.params(model, scheme, M=M3, N=N3, seed=SEED, stream=STREAM, pair_offset=OFF)
    jump = (tj.lam_of(N3), tj.MU, tj.SJ)
    thr, _, rj = _ffi.jump_table(p, jump, tj.Q)
    out, S = tj.priced(ctx, p, jump, tj.Q)
    V = tj.vanilla_at(ctx, p, rj)
    n, z = jr.draws(orc.philox4x32_10, M3 // 2, N3, SEED, STREAM, OFF, thr)
    ref = jr.apply(V, n, z, tj.MU, tj.SJ)
    ok, worst = dr.close(S, ref, ref, td.RTOL[model])
    assert ok, (model, scheme, worst)
    first = jr.first_jump_step(n)
    before = np.arange(N3 + 1)[:, None] < np.concatenate([first, first])[None, :]
    assert np.array_equal(bits(S)[before], bits(V)[before]) and (n > 0).any()
    td.check_price(out, S, p)


def test_basket_keeps_the_tagged_vanilla_matrices(ctx):
    """rho = I: asset k is the vanilla matrix at pair_offset + (k << 40) (tests/test_gpu_basket.py) -- here with the tag
    above a pair offset that carries into the pair counter's high word"""
    S0, sig, q, w, _, _ = tk.CASE8
    d = 3
    p = td.params(M=M3, N=N3, seed=SEED, stream=STREAM, pair_offset=OFF)
    _, S, A = tk.priced(ctx, p, _ffi.make_basket(S0[:d], sig[:d], q[:d], w[:d], np.eye(d), "basket"))
    for k in range(d):
        assert np.array_equal(bits(A[k]), bits(tk.vanilla(ctx, p, S0[k], p.r - q[k], sig[k], tag=k))), k
    from helpers import basket_ref
    assert np.abs(S / basket_ref.index(A, w[:d], "basket") - 1.0).max() <= d * 2.0 ** -23
    # correlated assets: the restatement on the oracle's normals at the tagged offsets
    b, _ = tk.basket_of(tk.CASE3, "basket")
    L, a, bb, _, _ = _ffi.basket_table(p, b)
    _, _, A = tk.priced(ctx, p, b)
    zs = [orc.gbm_normals(M3 // 2, N3, SEED, STREAM, OFF + (k << 40)) for k in range(3)]
    ref = basket_ref.assets(zs, tk.CASE3[0], a, bb, L)
    for k in range(3):
        ok, worst = dr.close(A[k], ref[k], ref[k], tk.RTOL)
        assert ok, (k, worst)


# ------------------------------------------------------------------ 5. the price bounds: three simulations, three key splits
BOUNDS = dict(n_lower=2048, n_outer=32, n_inner=64)


def _bounds_params(model="gbm", N=6, **law):
    return td.params(model, 0, M=4096, N=N, seed=SEED, stream=STREAM, pair_offset=OFF, **law)


def test_bounds_equal_the_restatement_at_the_base_triple(ctx):
    """tests/test_gpu_bounds.py::test_device_equals_restatement at this key: policy fitted on the paths of p, lower paths of
    stream + 1, outer paths of stream + 2, inner pairs of stream + 3"""
    p, N = _bounds_params(), 6
    d = ctx.price_american_bounds(p, policy="textbook", want_q=True, want_samples=True, **BOUNDS)
    Sp = ctx.gbm_paths(p.n_paths, N, p.S0, p.r, p.sigma, p.T, SEED, STREAM, OFF)
    fit = ctx.lsm_poly(Sp, p.K, p.r, p.T, True, "textbook")
    Sp.free()
    np.testing.assert_array_equal(d["betas"][:, :3], fit["betas"])
    np.testing.assert_array_equal(d["betas"][:, 3], fit["nitm"])
    Sl = host(ctx.gbm_paths(BOUNDS["n_lower"], N, p.S0, p.r, p.sigma, p.T, SEED, STREAM + 1))
    So = host(ctx.gbm_paths(BOUNDS["n_outer"], N, p.S0, p.r, p.sigma, p.T, SEED, STREAM + 2))
    Z = host(ctx.gbm_normals(BOUNDS["n_outer"] * (N + 1) * BOUNDS["n_inner"] // 2, N, SEED, STREAM + 3))
    inner = bounds_ref.inner_from_normals(Z, So, BOUNDS["n_inner"], lambda z, s0: host(ctx.gbm_paths_from_normals(z, s0, p.r, p.sigma, p.T)))
    lo = bounds_ref.lower_bound(Sl, p.K, p.r, p.T, True, d["betas"])
    up = bounds_ref.upper_bound(So, inner, p.K, p.r, p.T, True, d["betas"])
    assert lo["ties"] == 0 and up["ties"] == 0
    assert (d["n_exercised_lower"], d["inner_path_steps"]) == (lo["n_exercised"], up["inner_path_steps"])
    np.testing.assert_allclose(d["q"], up["q"], rtol=1e-12, atol=1e-12 * p.K)
    np.testing.assert_allclose(d["samples"], up["samples"], rtol=1e-12, atol=1e-12 * p.K)
    for k, ref in (("lower", lo), ("se_lower", lo), ("upper", up), ("se_upper", up)):
        assert d[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-12 * p.K), k


def test_heston_bounds_equal_the_restatement_at_the_base_triple(ctx):
    p = _bounds_params("heston", N=6, sigma=0.0)
    d = ctx.price_american_bounds_heston(p, policy="textbook", want_q=True, want_samples=True, **BOUNDS)
    np.testing.assert_array_equal(d["betas"], hc.fitted_table(ctx, p, "textbook"))
    sp = hc.device_spots(ctx, p, BOUNDS["n_lower"], BOUNDS["n_outer"], BOUNDS["n_inner"])
    hc.check_against_restatement(p, d, sp, BOUNDS["n_lower"], BOUNDS["n_outer"], BOUNDS["n_inner"])


@pytest.mark.parametrize("regressors", ["index", rr.REG])
def test_basket_bounds_equal_the_restatement_at_the_base_triple(ctx, regressors):
    p, b = _bounds_params(is_put=False), bc.unequal_basket(3, "best-of")
    dev = ctx.price_american_basket_bounds(p, b, policy="textbook", want_q=True, want_samples=True, regressors=regressors, **BOUNDS)
    if regressors == "index":
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, b, "textbook"))
    check = bc.check_against_restatement if regressors == "index" else rr.check_against_restatement
    lo, up = check(ctx, p, b, dev, BOUNDS["n_lower"], BOUNDS["n_outer"], BOUNDS["n_inner"])
    assert up["inner_path_steps"] >= BOUNDS["n_outer"] * BOUNDS["n_inner"]

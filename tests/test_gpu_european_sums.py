"""The European sums and standard errors of the three kernel families that return them, against the float64 restatement
of tests/helpers/european_ref.py on the device's OWN terminal spots:

  a. terminal_body<MODEL, ANTI> + lsm_finalize      omc_price_european and its batch: sum, sumsq, std, n_zero, zero_prob
  b. barrier_paths_body + barrier_finalize_kernel   omc_price_barrier: euro_out / euro_in, both standard errors, hit_prob,
                                                    and base when american = 0
  c. payoff_chunk_body + payoff_final_kernel        omc_heston_price_strikes / _surface: every price and every stderr

A register-only kernel never stores the terminal spots it saw, so each test regenerates them with the stored generator on
the same (seed, stream, pair_offset, rate) and takes the last row: terminal_body, heston_terminal_pair and the barrier
body run the stored generators' step on normals4 at the same counters, so the spots are the same bits (DESIGN.md
sections 4 and 11; tests/test_gpu_barrier.py observes it for the barrier body).  Were they not, a sum would miss by about
1e-5 of itself, far outside european_ref.sums_close.

The two bounds (european_ref.sums_close, se_close; derived in their docstrings) leave room for the order of a float64 sum
and for nothing else: a lost last element of a ragged chunk, a square added to the wrong slot, an M - 1 for an M, a
knock-in payoff counted as knock-out for one VEC layout all miss them by orders of magnitude
(tests/test_european_ref_cpu.py shows that at every shape used here).

Shapes: the smallest at which each layout of a kernel can go wrong; tests/test_european_ref_cpu.py derives the layouts
from the kernels' constants and asserts that the lists below hold every one of them."""
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import barrier_ref as br
from helpers import european_ref as er
from oracle import cpu as orc
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

S0, K, R, SIG, T = 100.0, 100.0, 0.05, 0.2, 1.0
HES = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
SEED, OFFSET = 20240611, 321

# ---- a. omc_price_european: (name, model, Heston scheme, antithetic)
EURO_MODELS = [("gbm-anti", "gbm", 0, True), ("gbm-single", "gbm", 0, False), ("heston0", "heston", 0, True),
               ("heston1", "heston", 1, True), ("heston2", "heston", 2, True)]
EURO_N = [1, 4, 5, 9]            # end on and inside a Philox block (4 steps per block for GBM, 2 for Heston)
EURO_M = [2, 254, 512, 514, 4098]
EURO_M_SINGLE = [2, 127, 256, 257, 513, 2049]   # non-antithetic: a work item is one path; 513 and 2049 are odd
EURO_BIG = (524_802, 3)          # P = 262,401 = 1024 x 256 + 257: the grid-stride loop's second trip, 257 lanes only
EURO_BIG_SINGLE = (262_401, 3)

# ---- b. omc_price_barrier: (name, model, Heston scheme, monitoring)
BARRIER_MODELS = [("gbm-discrete", "gbm", 0, "discrete"), ("gbm-continuous", "gbm", 0, "continuous"),
                  ("heston0", "heston", 0, "discrete"), ("heston1", "heston", 1, "discrete"),
                  ("heston2", "heston", 2, "discrete")]
BARRIER_N = [5, 9]
BARRIER_M = [2, 8, 1026, 2048, 2056]
BARRIER_BIG = (131_074, 5)       # P = 65,537, odd: VEC 1, 257 partials, the finalize loop's second trip for one thread
H_DOWN, H_UP = 90.0, 112.0

# ---- c. omc_heston_price_strikes / _surface
STRIKE_N = [1, 2, 7]
STRIKE_M = [2, 254, 4096, 4098, 8190, 12_290]
STRIKE_COUNTS = [1, 3, 61]
SURFACE_M = 4098                 # padded_ld(4098) = 4160: a chunk must stop at M, not at the row's stride


def _params(model, scheme, is_put, M, N, stream, antithetic=True, pair_offset=OFFSET, seed=SEED, law=None):
    """(law: a Heston law in place of HES -- tests/test_gpu_heston_qe_consumers.py passes the laws of the QE scheme)"""
    return _ffi.make_params(model=model, heston_scheme=scheme, is_put=is_put, semantics="two_pass", antithetic=antithetic,
                            n_paths=M, n_steps=N, S0=S0, K=K, r=R, sigma=SIG, T=T, seed=seed, stream=stream,
                            pair_offset=pair_offset, **(law or HES))


def _matrix(ctx, p):
    """the stored generator's matrix [N + 1][M] on the coordinates of p"""
    if p.model == 1:
        S = ctx.heston_paths(p.n_paths, p.n_steps, p.S0, p.r, p.T, p.v0, p.kappa, p.theta, p.xi, p.rho, p.seed, p.stream,
                             p.pair_offset, scheme=p.heston_scheme)
    else:
        S = ctx.gbm_paths(p.n_paths, p.n_steps, p.S0, p.r, p.sigma, p.T, p.seed, p.stream, p.pair_offset,
                          antithetic=bool(p.antithetic))
    out = S.to_host()
    S.free()
    assert np.isfinite(out).all()
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ a. omc_price_european
def _check_european(res, ST, is_put, what):
    M = ST.size
    ref = er.sums(ST, K, math.exp(-R * T), is_put, True)
    assert 0 < ref["n_zero"] < M or M <= 2, what  # both branches of p > 0 are taken
    er.sums_close(res["sum"], ref["sum"], ref["sum_abs"], M)
    er.sums_close(res["sumsq"], ref["sumsq"], ref["sumsq"], M)
    assert (res["n_zero"], res["n_paths"]) == (ref["n_zero"], M), what
    assert res["price"] == res["sum"] / M and res["zero_prob"] == ref["n_zero"] / M, what
    # std = sqrt(var) = se sqrt(M): the same variance bound
    er.se_close(res["std"], ref["sum"], ref["sumsq"], M, scale=np.sqrt(np.longdouble(M)))
    assert res["n_exercised"] == 0 and res["sum_nitm"] == 0, what


def _european_cases(model, anti):
    for N in EURO_N:
        for M in (EURO_M if anti else EURO_M_SINGLE):
            yield M, N
    yield EURO_BIG if anti else EURO_BIG_SINGLE


@pytest.mark.parametrize("name,model,scheme,anti", EURO_MODELS, ids=[m[0] for m in EURO_MODELS])
def test_price_european_sums_against_the_restatement(ctx, name, model, scheme, anti):
    for M, N in _european_cases(model, anti):
        V = _matrix(ctx, _params(model, scheme, True, M, N, stream=3, antithetic=anti))
        for is_put in (True, False):
            p = _params(model, scheme, is_put, M, N, stream=3, antithetic=anti)
            _check_european(ctx.price_european(p), V[-1], is_put, (name, M, N, is_put))


@pytest.mark.parametrize("name,model,scheme,anti", EURO_MODELS, ids=[m[0] for m in EURO_MODELS])
def test_price_european_batch_sums_against_the_restatement(ctx, name, model, scheme, anti):
    """the shared-launch body (terminal_body behind the batch's table) and the batch's finalize: problems of several
    shapes and both sides in one batch (a batch shares model, scheme and antithetic)"""
    shapes = [(514, 5), (4098, 9), (254, 4), (2, 1)] if anti else [(513, 5), (2049, 9), (127, 4), (2, 1)]
    ps = [_params(model, scheme, i % 2 == 0, M, N, stream=4 + i, antithetic=anti) for i, (M, N) in enumerate(shapes)]
    out = ctx.price_european_batch(ps)
    assert len(out) == len(ps)
    for p, res in zip(ps, out):
        _check_european(res, _matrix(ctx, p)[-1], bool(p.is_put), (name, p.n_paths, p.n_steps))
        one = ctx.price_european(p)
        assert (res["sum"], res["sumsq"], res["n_zero"], res["std"]) == (one["sum"], one["sumsq"], one["n_zero"], one["std"])


# ------------------------------------------------------------------ b. the barrier sums
EURO_KEYS = ("euro_out", "euro_out_se", "euro_in", "euro_in_se", "hit_prob")


def _kept(ctx, p, kind, H, monitoring):
    keep = ctx.empty((p.n_steps + 1, p.n_paths), np.float32)
    ctx.price_barrier(p, kind, H, monitoring=monitoring, american=False, keep_paths=keep)
    S = keep.to_host()
    keep.free()
    return S


def _hit_set(ctx, p, V, direction, H, monitoring):
    """per path: did it hit?  Discrete: the documented float64 test on the vanilla matrix.  Continuous: from a knock-out
    run's kept matrix -- hit where any row 1..N differs in bits from the vanilla matrix (a knock-out is dead at its hit
    step and after it; the knock-in of the same barrier shares the set: both partners share u_t, the kinds the test)."""
    N = p.n_steps
    discrete = br.discrete_hit_steps(V, direction + "-and-out", H) <= N
    if monitoring == "discrete":
        return discrete
    S = _kept(ctx, p, direction + "-and-out", H, "continuous")
    assert np.array_equal(_bits(S[0]), _bits(V[0]))
    hit = np.any(_bits(S[1:]) != _bits(V[1:]), axis=0)
    assert np.all(hit[discrete])  # continuous monitoring hits wherever discrete monitoring does
    return hit


def _check_barrier(ctx, p, V, kind, H, monitoring, ref, what):
    """all five European fields of both styles against barrier_sums' `ref`, base of the European style"""
    M = p.n_paths
    runs = {am: ctx.price_barrier(p, kind, H, monitoring=monitoring, american=am) for am in (False, True)}
    eu, am = runs[False], runs[True]
    assert tuple(eu[k] for k in EURO_KEYS) == tuple(am[k] for k in EURO_KEYS), what
    for side in ("out", "in"):
        r = ref[side]
        er.sums_close(Fraction(eu["euro_" + side]) * M, r["sum"], r["sum_abs"], M)
        er.se_close(eu[f"euro_{side}_se"], r["sum"], r["sumsq"], M)
    assert eu["hit_prob"] == ref["hit_prob"], what
    own = ref["in" if kind.endswith("-in") else "out"]
    er.sums_close(eu["sum"], own["sum"], own["sum_abs"], M)
    er.sums_close(eu["sumsq"], own["sumsq"], own["sumsq"], M)
    er.se_close(eu["std"], own["sum"], own["sumsq"], M, scale=np.sqrt(np.longdouble(M)))
    assert eu["price"] == eu["sum"] / M == eu["euro_in" if kind.endswith("-in") else "euro_out"], what
    assert (eu["n_paths"], eu["n_zero"], eu["zero_prob"], eu["n_exercised"]) == (M, 0, 0.0, 0), what
    return eu


def _barrier_shape(ctx, model, scheme, monitoring, M, N, stream=13, law=None, levels=(H_DOWN, H_UP)):
    df = math.exp(-R * T)
    V = _matrix(ctx, _params(model, scheme, True, M, N, stream, law=law))
    seen = []
    for direction, H in (("down", levels[0]), ("up", levels[1])):
        hit = _hit_set(ctx, _params(model, scheme, True, M, N, stream, law=law), V, direction, H, monitoring)
        seen.append(int(hit.sum()))
        for is_put in (True, False):
            ref = er.barrier_sums(V[-1], hit, K, df, is_put)
            p = _params(model, scheme, is_put, M, N, stream, law=law)
            for kind in (direction + "-and-out", direction + "-and-in"):
                _check_barrier(ctx, p, V, kind, H, monitoring, ref, (model, scheme, monitoring, M, N, kind, is_put))
    return seen


@pytest.mark.parametrize("M", BARRIER_M)
@pytest.mark.parametrize("name,model,scheme,monitoring", BARRIER_MODELS, ids=[m[0] for m in BARRIER_MODELS])
def test_barrier_sums_against_the_restatement(ctx, name, model, scheme, monitoring, M):
    for N in BARRIER_N:
        seen = _barrier_shape(ctx, model, scheme, monitoring, M, N)
        assert M < 1000 or all(0 < h < M for h in seen), (name, M, N, seen)  # both columns are fed


@pytest.mark.parametrize("name,model,scheme,monitoring", BARRIER_MODELS, ids=[m[0] for m in BARRIER_MODELS])
def test_barrier_sums_where_the_finalize_loop_takes_a_second_trip(ctx, name, model, scheme, monitoring):
    M, N = BARRIER_BIG
    seen = _barrier_shape(ctx, model, scheme, monitoring, M, N)
    assert all(0 < h < M for h in seen), seen


def test_barrier_no_path_hits(ctx):
    """inputs chosen on the CPU oracle's spots with margin: every spot is more than 1e-3 (relative) inside the barriers"""
    M, N, stream = 2056, 5, 17
    Vo = orc.gbm_paths(M, N, S0, R, SIG, T, SEED, stream, OFFSET).astype(np.float64)
    for direction, H in (("down", 20.0), ("up", 500.0)):
        assert (Vo[1:].min() > H * (1 + 1e-3)) if direction == "down" else (Vo[1:].max() < H * (1 - 1e-3))
        for monitoring in ("discrete", "continuous"):
            p = _params("gbm", 0, direction == "down", M, N, stream)
            V = _matrix(ctx, p)
            hit = _hit_set(ctx, p, V, direction, H, monitoring)
            assert not hit.any()
            ref = er.barrier_sums(V[-1], hit, K, math.exp(-R * T), bool(p.is_put))
            for kind in (direction + "-and-out", direction + "-and-in"):
                eu = _check_barrier(ctx, p, V, kind, H, monitoring, ref, (direction, monitoring, kind))
                assert (eu["euro_in"], eu["euro_in_se"], eu["hit_prob"]) == (0.0, 0.0, 0.0)
                assert eu["euro_out"] > 0.0 and eu["euro_out_se"] > 0.0


def test_barrier_every_path_hits(ctx):
    """M = 8, streams found on the CPU oracle: every one of the 8 paths passes the barrier by more than 1e-3 (relative)"""
    M, N = 8, 9
    for direction, H, stream in (("down", 96.0, 2060), ("up", 108.0, 931)):
        Vo = orc.gbm_paths(M, N, S0, R, SIG, T, 42, stream, 0).astype(np.float64)
        far = Vo[1:].min(axis=0).max() < H * (1 - 1e-3) if direction == "down" else Vo[1:].max(axis=0).min() > H * (1 + 1e-3)
        assert far
        for is_put in (True, False):
            p = _params("gbm", 0, is_put, M, N, stream, pair_offset=0, seed=42)
            V = _matrix(ctx, p)
            hit = _hit_set(ctx, p, V, direction, H, "discrete")
            assert hit.all()
            ref = er.barrier_sums(V[-1], hit, K, math.exp(-R * T), is_put)
            for kind in (direction + "-and-out", direction + "-and-in"):
                eu = _check_barrier(ctx, p, V, kind, H, "discrete", ref, (direction, is_put, kind))
                assert (eu["euro_out"], eu["euro_out_se"], eu["hit_prob"]) == (0.0, 0.0, 1.0)


def test_barrier_threshold_not_representable_in_float32(ctx):
    """H whose float32 neighbour lies on the wrong side: barrier_threshold steps one ulp (down: (float)H > H, up: (float)H
    < H), and the float32 comparison is still the documented float64 test"""
    M, N, stream = 2056, 9, 19
    for direction, H in (("down", 90.3), ("up", 112.1)):
        Hf = float(np.float32(H))
        assert Hf > H if direction == "down" else Hf < H
        for model, scheme in (("gbm", 0), ("heston", 1)):
            p = _params(model, scheme, True, M, N, stream)
            V = _matrix(ctx, p)
            hit = _hit_set(ctx, p, V, direction, H, "discrete")
            assert 0 < hit.sum() < M
            ref = er.barrier_sums(V[-1], hit, K, math.exp(-R * T), True)
            for kind in (direction + "-and-out", direction + "-and-in"):
                _check_barrier(ctx, p, V, kind, H, "discrete", ref, (direction, model, kind))


# ------------------------------------------------------------------ c. the strike kernels
def _strikes(row, is_put, count):
    """far in the money (every payoff positive), far out (price and se exactly 0), the exact float64 value of a terminal
    spot (payoff exactly 0 on the p > 0 edge), near the money; 61: a ladder besides"""
    far_in, far_out = (1000.0, 1.0) if is_put else (1.0, 1000.0)
    spot = float(row[row.size // 3])
    if count == 1:
        return np.array([spot])
    if count == 3:
        return np.array([far_in, far_out, spot])
    return np.concatenate([[far_in, far_out, 100.5, spot], np.linspace(80.0, 120.0, count - 4)])


def _check_quotes(prices, errs, strikes, row, df, is_put, what):
    M = row.size
    assert 1.0 < row.min() and row.max() < 1000.0, what  # what `far` assumes
    for k, price, err in zip(strikes, prices, errs):
        ref = er.sums(row, float(k), df, is_put, False)
        er.sums_close(Fraction(float(price)) / Fraction(df), Fraction(ref["sum"]) / M, Fraction(ref["sum_abs"]) / M, M)
        er.se_close(float(err), ref["sum"], ref["sumsq"], M, scale=df)
        if ref["n_zero"] == M:
            assert price == 0.0 and err == 0.0, what
        if ref["n_zero"] == 0:
            assert price > 0.0, what
    return True


def _row(ctx, M, N, Texp, scheme, stream, seed=SEED, law=None):
    h = law or HES
    S = ctx.heston_paths(M, N, S0, R, Texp, h["v0"], h["kappa"], h["theta"], h["xi"], h["rho"], seed, stream, 0,
                         scheme=scheme)
    out = S.to_host()[-1].copy()
    S.free()
    return out


@pytest.mark.parametrize("M", STRIKE_M)
@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_strike_prices_and_stderrs_against_the_restatement(ctx, scheme, M):
    h = HES
    for N in STRIKE_N:
        row = _row(ctx, M, N, T, scheme, stream=23)
        for is_put in (True, False):
            for count in STRIKE_COUNTS:
                ks = _strikes(row, is_put, count)
                prices, errs = ctx.heston_price_strikes(M, N, S0, R, T, h["v0"], h["kappa"], h["theta"], h["xi"], h["rho"], ks,
                                                        is_put=is_put, seed=SEED, stream=23, scheme=scheme)
                assert _check_quotes(prices, errs, ks, row, math.exp(-R * T), is_put, (scheme, M, N, is_put, count))
                spot = ks[0 if count == 1 else (2 if count == 3 else 3)]
                assert er.sums(row, float(spot), 1.0, is_put, False)["n_zero"] >= 1  # the p > 0 edge is met


@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_surface_prices_and_stderrs_against_each_expiry_row(ctx, scheme):
    """three expiries, quotes in shuffled order: the rows of the spot buffer are padded_ld(M) apart, so a chunk that ran to
    the stride instead of M would add the padding or the next expiry's spots"""
    h, M, N = HES, SURFACE_M, 7
    expiries, streams = [0.25, 0.5, 1.0], [31, 32, 33]
    rows = [_row(ctx, M, N, Te, scheme, stream=s) for Te, s in zip(expiries, streams)]
    rng = np.random.default_rng(5)
    for is_put in (True, False):
        ks = np.concatenate([_strikes(r, is_put, 8) for r in rows])
        eo = np.repeat(np.arange(3), 8)
        order = rng.permutation(ks.size)
        ks, eo = ks[order], eo[order]
        prices, errs = ctx.heston_price_surface(M, N, S0, R, h["v0"], h["kappa"], h["theta"], h["xi"], h["rho"], expiries,
                                                streams, ks, eo, is_put=is_put, seed=SEED, scheme=scheme)
        for e in range(3):
            sel = eo == e
            assert _check_quotes(prices[sel], errs[sel], ks[sel], rows[e], math.exp(-R * expiries[e]), is_put,
                                 (scheme, "surface", e, is_put))

"""Andersen-Broadie price bounds for barrier options (omc_price_american_bounds_barrier, omc_barrier_paths_state_f32;
options_model_amd/csrc/omc_barrier_bounds.hip).

The generator that keeps the paths' state against omc_price_barrier's kept matrix, the vanilla generators and
tests/helpers/barrier_ref.py (bits), and restarted from its own state; the device's Q^_t, samples, bounds and counts against
the numpy restatement of tests/helpers/barrier_bounds_ref.py on the device's own REAL spots (tests/helpers/
barrier_bounds_case.py: built from the vanilla generators, so the code under test takes no part in its reference) for all four
kinds x put / call x GBM and Heston 0 / 1 x plain / scheduled / payoff-checked; the unreachable barrier against the vanilla
bounds, bit for bit; the never-exercising policy against omc_price_barrier's European sums; the dead items; the refusals;
determinism; the facade and the C example.  Every case at a small shape."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import barrier_bounds_case as bc
from helpers import barrier_bounds_ref as bbr
from helpers import barrier_ref as bar
from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu

K, R, SIG, T = 100.0, 0.05, 0.2, 1.0
OUT_KEYS = ("lower", "se_lower", "upper", "se_upper", "ci_lo", "ci_hi", "n_lower", "n_outer", "n_inner", "n_exercised_lower",
            "inner_path_steps")


def _params(model="gbm", is_put=True, S0=100.0, N=8, M=2000, seed=42, stream=0, hp=None):
    hp = hp or (bc.HP_CLAMP if model == "heston1" else bc.HP)  # scheme 1 with the Feller-violating set
    return bc.make_params(model, is_put=is_put, S0=S0, K=K, r=R, sigma=SIG, T=T, N=N, M=M, seed=seed, stream=stream, hp=hp)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b, keys=OUT_KEYS, arrays=("betas", "q", "samples")):
    for key in keys:
        assert a[key] == b[key], key
    for key in arrays:
        if key in a or key in b:
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def _state(ctx, p, kind, H, start_hit=False):
    """the state generator's four outputs on the host (V None under GBM)"""
    E, S, V, hit = ctx.barrier_paths_state(p, kind, H, start_hit=start_hit)
    return bc.host(E), bc.host(S), (bc.host(V) if V is not None else None), bc.host(hit)


# ---------------------------------------------------------------------------------------------- 1. the generator
@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("model", bc.MODELS)
@pytest.mark.parametrize("M,N", [(4096, 13), (1000, 7), (10, 3), (2, 1)])  # (the pricing call stores 4, 4, 1, 1 pairs wide)
def test_generator_against_the_pricing_call_the_vanilla_paths_and_the_encoder(ctx, model, kind, M, N):
    H = 94.0 if kind.startswith("down") else 106.0
    for is_put in (True, False):
        p = bc.with_(_params(model, is_put=is_put, S0=101.0, N=N, M=M, seed=9, stream=5), pair_offset=3)  # (S0 is not the dead spot)
        E, S, V, hit = _state(ctx, p, kind, H)
        np.testing.assert_array_equal(_bits(E), _bits(bc.barrier_fit_matrix(ctx, p, kind, H)))  # omc_price_barrier's S_keep
        if bc.is_heston(p):
            Sv, Vv = bc.vanilla_paths(ctx, p, want_v=True)
            np.testing.assert_array_equal(_bits(V), _bits(Vv))
        else:
            Sv = bc.vanilla_paths(ctx, p)
            assert V is None
        np.testing.assert_array_equal(_bits(S), _bits(Sv))
        assert hit.dtype == np.int32 and hit.shape == (M,)
        np.testing.assert_array_equal(hit, bbr.first_hit(S, kind, H))
        np.testing.assert_array_equal(_bits(E), _bits(bbr.encode(S, kind, H, K, is_put)[0]))
        # hit = the first row at which the encoding differs from the real spot (knock-out) / stops differing (knock-in)
        differs = _bits(E) != _bits(S)
        if bbr.knock_out(kind):
            first = np.where(differs.any(axis=0), differs.argmax(axis=0), 0)
        else:
            first = np.where(differs.all(axis=0), 0, (~differs).argmax(axis=0))
            assert differs[0].all()  # row 0 of a knock-in is dead
        np.testing.assert_array_equal(hit, first)
    if M >= 1000:
        assert 0.05 < np.count_nonzero(hit) / M < 0.95


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("model", bc.MODELS)
def test_state_restarts_the_path_with_the_hit_state_carried(ctx, model, kind):
    """(S[t, j], V[t, j], hit(t, j)) is the state after step t: the from-normals entry point started at the real spot and
    variance with the generator's remaining normals (padded to N rows, as tests/test_gpu_heston_bounds.py does it), encoded
    with the start's hit state, reproduces rows t .. N of that column of E bit for bit.  And the generator itself started hit
    (start_hit = 1, S0 anywhere): every row is encoded as hit and every entry of hit is -1."""
    M, N, stream, off = 600, 13, 5, 7
    P = M // 2
    H = 95.0 if kind.startswith("down") else 105.0
    p = bc.with_(_params(model, N=N, M=M, seed=21, stream=stream), pair_offset=off)
    E, S, V, hit = _state(ctx, p, kind, H)
    heston = bc.is_heston(p)
    Z = bc.host(ctx.gbm_normals(P, 2 * N if heston else N, p.seed, stream, off))
    hp = p.kappa, p.theta, p.xi, p.rho
    seen = set()
    for t in (0, 4, 12):
        was_hit = (hit != 0) & (hit <= t)
        picks = {0, 1, P - 1}
        for flag in (True, False):  # a pair with a partner hit by t and one with none, where there is one
            idx = np.flatnonzero((was_hit[:P] | was_hit[P:]) == flag)
            picks |= {int(idx[0])} if idx.size else set()
        for j in sorted(picks):
            for col, out_col in ((j, 0), (j + P, 1)):
                if heston:
                    pad1, pad2 = np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32)
                    pad1[:N - t, 0], pad2[:N - t, 0] = Z[0::2][t:, j], Z[1::2][t:, j]
                    X = bc.host(ctx.heston_paths_from_normals(pad1, pad2, float(S[t, col]), R, T, float(V[t, col]), *hp,
                                                              int(p.heston_scheme)))
                else:
                    pad = np.zeros((N, 1), np.float32)
                    pad[:N - t, 0] = Z[t:, j]
                    X = bc.host(ctx.gbm_paths_from_normals(pad, float(S[t, col]), R, SIG, T))
                X = X[:N - t + 1, out_col:out_col + 1]
                np.testing.assert_array_equal(_bits(X[:, 0]), _bits(S[t:, col]))
                enc = bbr.encode(X, kind, H, K, True, start_hit=bool(was_hit[col]))[0]
                np.testing.assert_array_equal(_bits(enc[:, 0]), _bits(E[t:, col]), err_msg=f"t {t} column {col}")
                seen.add(bool(was_hit[col]))
    assert seen == {True, False}
    for S0 in (100.0, 80.0, 120.0):  # on either side of the barrier: a start state, not refused
        E2, S2, V2, hit2 = _state(ctx, bc.with_(p, S0=S0), kind, H, start_hit=True)
        assert np.all(hit2 == -1)
        np.testing.assert_array_equal(_bits(E2), _bits(bbr.encode(S2, kind, H, K, True, start_hit=True)[0]))
        assert np.all(E2 == bar.dead_spot(K, True)) if bbr.knock_out(kind) else np.array_equal(_bits(E2), _bits(S2))


def test_generator_with_an_odd_leading_dimension_and_refusals(ctx):
    M, N, ld = 10, 5, 13
    for model in ("gbm", "heston1"):
        p = _params(model, N=N, M=M, seed=9)
        b = _ffi.make_barrier("down-and-out", 95.0)
        ref = _state(ctx, p, "down-and-out", 95.0)
        bufs = [ctx.to_device(np.full((N + 1, ld), np.float32(-7.0))) for _ in range(3)]
        hit = ctx.to_device(np.full((ld,), -7, np.int32))
        v = bufs[2].ptr if bc.is_heston(p) else None
        call = ctx.lib.omc_barrier_paths_state_f32
        assert call(ctx.handle, C.byref(p), C.byref(b), 0, bufs[0].ptr, bufs[1].ptr, v, hit.ptr, ld) == 0
        got = [bc.host(x) for x in bufs]
        h = bc.host(hit)
        for a, r in zip(got, ref[:3]):
            if r is not None:
                np.testing.assert_array_equal(_bits(a[:, :M]), _bits(r))
            assert np.all(a[:, M:] == -7.0)  # (the padding is not written)
        np.testing.assert_array_equal(h[:M], ref[3])
        assert np.all(h[M:] == -7)
    p = _params("gbm", N=N, M=M)
    h = _params("heston0", N=N, M=M)
    E, S, V = (ctx.empty((N + 1, M), np.float32) for _ in range(3))
    hit = ctx.empty((M,), np.int32)

    def rc(pp, kind=0, H=95.0, mon=0, start=0, e=E, s=S, v=None, ht=hit, ld=M, null_b=False):
        b = _ffi.make_barrier(kind, H, mon)
        return ctx.lib.omc_barrier_paths_state_f32(ctx.handle, C.byref(pp), None if null_b else C.byref(b), start,
                                                   e.ptr if e else None, s.ptr if s else None, v.ptr if v else None,
                                                   ht.ptr if ht else None, ld)

    assert rc(p) == 0 and rc(h, v=V) == 0
    assert rc(p, null_b=True) == -7 and rc(p, e=None) == -7 and rc(p, s=None) == -7 and rc(p, ht=None) == -7
    assert rc(p, v=V) == -7 and rc(h) == -7  # V under Heston and only there
    assert rc(p, kind=4) == -15 and rc(p, kind=-1) == -15 and rc(p, mon=2) == -15 and rc(p, start=2) == -15
    assert rc(bc.with_(p, antithetic=0)) == -15
    assert rc(p, mon=1) == -12  # continuous monitoring
    for scheme in (2, 3):
        assert rc(bc.with_(h, heston_scheme=scheme), v=V) == -12
    assert rc(p, H=0.0) == -13 and rc(p, H=float("nan")) == -13
    assert rc(p, H=100.0) == -14 and rc(p, H=105.0) == -14 and rc(p, kind=1, H=100.0) == -14 and rc(p, kind=3, H=95.0) == -14
    assert rc(p, H=105.0, start=1) == 0  # a start state may lie beyond the barrier
    assert rc(p, ld=M - 1) == -6
    assert rc(bc.with_(h, v0=-0.01), v=V) == 0  # a stored full-truncation state
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        b = _ffi.make_barrier(0, 95.0)
        assert hooked.lib.omc_barrier_paths_state_f32(hooked.handle, C.byref(p), C.byref(b), 0, E.ptr, S.ptr, None, hit.ptr,
                                                      M) == -10
    finally:
        hooked.close()
    for a in (E, S, V, hit):
        a.free()


# ---------------------------------------------------------------------------------------------- 2. the restatement
_spots = {}


def _shape_spots(ctx, name):
    """the device's own REAL spots of a shape, computed once: they depend on the law and the sizes alone"""
    if name not in _spots:
        s = bc.SHAPES[name]
        _spots[name] = bc.device_spots(ctx, bc.shape_params(s), s["n_lower"], s["n_outer"], s["n_inner"])
    return _spots[name]


@pytest.mark.parametrize("c", bc.CASES, ids=[bc.case_id(c) for c in bc.CASES])
def test_device_equals_restatement(ctx, c):
    s = bc.SHAPES[c["shape"]]
    kind, H = c["kind"], bc.barrier_of(s, c["kind"])
    p = bc.shape_params(s, is_put=c["is_put"])
    every, check = bc.mode_args(s, c["mode"])
    sizes = (s["n_lower"], s["n_outer"], s["n_inner"])
    betas = bc.given_table(ctx, p, bc.holes_of(s["N"])) if c["policy"] == "given" else None
    dev = ctx.price_barrier_bounds(p, kind, H, policy=c["policy"], n_lower=sizes[0], n_outer=sizes[1], n_inner=sizes[2],
                                   betas=betas, want_q=True, want_samples=True, exercise_every=every, suboptimality_check=check)
    if c["policy"] != "given":  # the fit is omc_lsm_poly's on omc_price_barrier's encoded matrix
        np.testing.assert_array_equal(dev["betas"], bc.fitted_table(ctx, p, kind, H, c["policy"], every))
    sp = _shape_spots(ctx, c["shape"])
    lo, up = bbr.check_against_restatement(p, dev, sp, kind, H, every, check, *sizes)
    # the dead items of a knock-out: Q^ = 0.0 exactly (and, being skipped, they are no part of the step count above)
    dead = bbr.dead_items(up["hit"], s["N"], kind).T
    assert np.all(dev["q"][dead] == 0.0) and not np.signbit(dev["q"][dead]).any()
    if bbr.knock_out(kind) and s["N"] > 1:
        assert dead.any() and not dead.all()
    assert dev["upper"] >= dev["lower"] - 3.0 * (dev["se_lower"] + dev["se_upper"])
    assert dev["lower"] >= 0.0 and dev["upper"] >= 0.0


# ---------------------------------------------------------------------------------------------- 3. degenerate contracts
@pytest.mark.parametrize("mode", bc.MODES)
@pytest.mark.parametrize("model", bc.MODELS)
def test_unreachable_knock_out_carries_the_vanilla_bits(ctx, model, mode):
    """every output but the timings, betas_out included: the fit's matrix, the paths, the list-driven sweep with every item
    kept and the walk over every date all carry the vanilla call's bits"""
    N = 7
    every, check = (3, None) if mode == "scheduled" else (0, "payoff" if mode == "payoff" else None)
    kw = dict(n_lower=1000, n_outer=22, n_inner=130, want_q=True, want_samples=True, exercise_every=every,
              suboptimality_check=check)
    for is_put, policy in ((True, "textbook"), (False, "two_pass")):
        p = _params(model, is_put=is_put, N=N, seed=5)
        ref = ctx.price_american_bounds_heston(p, policy=policy, **kw) if bc.is_heston(p) else \
            ctx.price_american_bounds(p, policy=policy, **kw)
        for kind in ("down-and-out", "up-and-out"):
            _same_bits(ctx.price_barrier_bounds(p, kind, bc.unreachable(kind), policy=policy, **kw), ref)


@pytest.mark.parametrize("model", bc.MODELS)
def test_unreachable_knock_in_is_worth_nothing(ctx, model):
    p = _params(model, N=7, seed=5)
    table = bc.given_table(ctx, p)
    for kind in ("down-and-in", "up-and-in"):
        for policy, betas in (("textbook", None), ("given", table)):
            d = ctx.price_barrier_bounds(p, kind, bc.unreachable(kind), policy=policy, betas=betas, n_lower=1000, n_outer=22,
                                         n_inner=130, want_q=True, want_samples=True)
            assert (d["lower"], d["upper"], d["se_lower"], d["se_upper"], d["n_exercised_lower"]) == (0.0, 0.0, 0.0, 0.0, 0)
            assert np.all(d["q"] == 0.0) and np.all(d["samples"] == 0.0)
            assert d["inner_path_steps"] == 22 * 130 * 7 * 8 // 2  # nothing stops before N


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("model", bc.MODELS)
def test_never_exercising_policy_gives_the_european_barrier_value(ctx, model, kind):
    """policy `given` with n = 0 on every date: a path stops at N or where it is knocked out, so `lower` is the European
    option of `kind` on the lower paths -- omc_price_barrier's euro_out / euro_in at (n_lower, stream_lower)"""
    N, n_lower = 13, 1400
    H = 93.0 if kind.startswith("down") else 107.0
    for is_put in (True, False):
        p = _params(model, is_put=is_put, N=N, seed=8, stream=3)
        d = ctx.price_barrier_bounds(p, kind, H, policy="given", betas=bbr.never_exercise_table(N), n_lower=n_lower, n_outer=2,
                                     n_inner=2, stream_lower=11)
        e = ctx.price_barrier(bc.with_(p, n_paths=n_lower, stream=11), kind, H, american=False)
        want = e["euro_in"] if kind.endswith("-in") else e["euro_out"]
        assert 0.02 < e["hit_prob"] < 0.98
        assert abs(d["lower"] - want) <= 1e-12 * K, (d["lower"], want)
        # a knocked-out path counts as stopped before N where it is hit before N; a knock-in never stops early
        S = bc.vanilla_paths(ctx, bc.with_(p, n_paths=n_lower, stream=11))
        early = int(np.count_nonzero(bar.discrete_hit_steps(S, kind, H) < N)) if bbr.knock_out(kind) else 0
        assert d["n_exercised_lower"] == early


# ---------------------------------------------------------------------------------------------- 4. the steps saved
@pytest.mark.parametrize("model", bc.MODELS)
def test_knocked_out_lanes_stop_at_the_hit(ctx, model):
    """with a policy that never exercises every inner path of the vanilla call runs to N; the knock-out's run to their hit
    step, and the dead items run not at all: the step count is the restatement's, far below the vanilla call's"""
    N, n_outer, n_inner = 7, 22, 130
    p = _params(model, N=N, seed=6)
    kw = dict(policy="given", betas=bbr.never_exercise_table(N), n_lower=600, n_outer=n_outer, n_inner=n_inner, want_q=True)
    full = n_outer * n_inner * N * (N + 1) // 2
    ko = ctx.price_barrier_bounds(p, "down-and-out", 97.0, **kw)
    ki = ctx.price_barrier_bounds(p, "down-and-in", 97.0, **kw)
    assert ki["inner_path_steps"] == full and 0 < ko["inner_path_steps"] < 0.7 * full
    sp = bc.device_spots(ctx, p, 600, n_outer, n_inner)
    up = bbr.upper_bound(sp["So"], sp["inner"], "down-and-out", 97.0, K, R, T, True, kw["betas"])
    assert ko["inner_path_steps"] == up["inner_path_steps"]
    dead = bbr.dead_items(up["hit"], N, "down-and-out").T
    assert dead.any() and np.all(ko["q"][dead] == 0.0)


# ---------------------------------------------------------------------------------------------- 5. refusals
SENTINEL = 0xAB


def _raw(ctx, p, kind=0, H=95.0, mon=0, policy=1, regressors=0, n_lower=1000, n_outer=6, n_inner=64, betas=None, null=()):
    """the C call with sentinel-filled outputs -> (rc, outputs untouched?)"""
    N = int(p.n_steps)
    cfg = _ffi.BoundsConfig()
    cfg.policy, cfg.regressors, cfg.n_lower, cfg.n_outer, cfg.n_inner = policy, regressors, n_lower, n_outer, n_inner
    cfg.stream_lower, cfg.stream_outer, cfg.stream_inner = 1, 2, 3
    out = _ffi.Bounds()
    C.memset(C.byref(out), SENTINEL, C.sizeof(out))
    bo, qo, so = (np.full(shape, np.nan) for shape in ((N + 1, 4), (max(n_outer, 1), N), (max(n_outer, 1),)))
    bar_ = _ffi.make_barrier(kind, H, mon)
    b = None if betas is None else np.ascontiguousarray(betas, np.float64)
    rc = ctx.lib.omc_price_american_bounds_barrier(ctx.handle, C.byref(p), None if "barrier" in null else C.byref(bar_),
                                                   None if "cfg" in null else C.byref(cfg),
                                                   b.ctypes.data if b is not None else None, bo.ctypes.data, qo.ctypes.data,
                                                   so.ctypes.data, None if "out" in null else C.byref(out))
    untouched = bytes(out) == bytes([SENTINEL]) * C.sizeof(out) and all(np.isnan(a).all() for a in (bo, qo, so))
    return rc, untouched


def test_refusals_leave_the_outputs_alone(ctx):
    p = _params("gbm")
    h = _params("heston0")
    nan = float("nan")
    cases = [(dict(null=("cfg",)), -7), (dict(null=("out",)), -7), (dict(null=("barrier",)), -7), (dict(kind=4), -15),
             (dict(kind=-1), -15), (dict(mon=2), -15), (dict(mon=1), -12), (dict(H=0.0), -13), (dict(H=nan), -13),
             (dict(H=100.0), -14), (dict(H=101.0), -14), (dict(kind=1, H=100.0), -14), (dict(kind=3, H=99.0), -14),
             (dict(regressors=1), -4), (dict(policy=7), -4), (dict(policy=3), -7), (dict(n_inner=63), -3),
             (dict(n_outer=7), -3), (dict(n_lower=999), -3),
             # the contract's errors come before the bounds' own
             (dict(H=nan, policy=7), -13), (dict(H=100.0, n_inner=63), -14), (dict(mon=1, policy=3), -12)]
    for kw, code in cases:
        for pp in (p, h):
            rc, untouched = _raw(ctx, pp, **kw)
            assert rc == code and untouched, (kw, rc)
    assert _raw(ctx, bc.with_(p, antithetic=0)) == (-15, True)
    assert _raw(ctx, bc.with_(p, sigma=0.0))[0] == -5
    for scheme in (2, 3):
        assert _raw(ctx, bc.with_(h, heston_scheme=scheme)) == (-12, True)
    assert _raw(ctx, _params("gbm", N=252), n_outer=1 << 14, n_inner=1 << 12) == (-16, True)
    assert _raw(ctx, bc.with_(p, semantics=0))[0] == 0  # p->semantics is not used
    hooked = _ffi.Context(0)
    try:
        hooked.set_allreduce_hook(lambda dptr, count: None)
        assert _raw(hooked, p) == (-10, True)
        assert _raw(hooked, p, H=nan) == (-13, True)
    finally:
        hooked.close()


def test_option_refusals_and_the_way_back(ctx):
    kw = dict(n_lower=1000, n_outer=6, n_inner=64, want_q=True, want_samples=True)
    pairs = [(_params(m), m) for m in bc.MODELS]
    before = {m: ctx.price_barrier_bounds(p, "down-and-out", 95.0, **kw) for p, m in pairs}
    try:
        ctx.set_option("bounds_control_variate", 1)
        for p, m in pairs:
            assert _raw(ctx, p) == (-12, True), m
            assert b"bounds_control_variate" in ctx.lib.omc_last_error()
            assert _raw(ctx, p, H=100.0) == (-14, True)  # the call's own checks come first
        ctx.set_option("bounds_control_variate", 0)
        ctx.set_option("bounds_suboptimality", 2)
        for p, m in pairs:
            assert _raw(ctx, p) == (-12, True), m
            assert b"bounds_suboptimality" in ctx.lib.omc_last_error()
        ctx.set_option("bounds_suboptimality", 1)
        ctx.set_option("bounds_exercise_every", 2)
        for p, m in pairs:
            assert _raw(ctx, p) == (-40, True), m  # a schedule and a check exclude each other
        ctx.set_option("bounds_exercise_every", 0)
        assert _raw(ctx, pairs[0][0])[0] == 0
    finally:
        ctx.set_option("bounds_exercise_every", 0)
        ctx.set_option("bounds_control_variate", 0)
        ctx.set_option("bounds_suboptimality", 0)
    assert (ctx._bounds_check, ctx._bounds_every, ctx._bounds_cv) == (0, 0, 0)
    for p, m in pairs:
        ctx.price_barrier_bounds(p, "down-and-out", 95.0, exercise_every=3, **kw)
        ctx.price_barrier_bounds(p, "up-and-in", 105.0, suboptimality_check="payoff", **kw)
        _same_bits(ctx.price_barrier_bounds(p, "down-and-out", 95.0, **kw), before[m])  # a plain call returns its old bits


# ---------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("kind", ("down-and-out", "up-and-in"))
@pytest.mark.parametrize("model", bc.MODELS)
def test_deterministic_and_table_fallback(ctx, model, kind):
    p = _params(model, N=13, M=4000)
    H = 94.0 if kind.startswith("down") else 106.0
    kw = dict(n_lower=1400, n_outer=40, n_inner=200, want_q=True, want_samples=True)
    a = ctx.price_barrier_bounds(p, kind, H, **kw)
    b = ctx.price_barrier_bounds(p, kind, H, **kw)
    ctx.set_option("pass2_tables_irregular_every", 2)  # every other step decided by the float64 rule: the same decisions
    try:
        c = ctx.price_barrier_bounds(p, kind, H, **kw)
    finally:
        ctx.set_option("pass2_tables_irregular_every", 0)
    _same_bits(b, a)
    _same_bits(c, a)
    ctx.price_barrier(p, "up-and-out", 120.0)  # (another contract through the context's buffers in between)
    _same_bits(ctx.price_barrier_bounds(p, kind, H, **kw), a)
    fresh = _ffi.Context(0)
    try:
        _same_bits(fresh.price_barrier_bounds(p, kind, H, **kw), a)  # and on a context that has seen nothing else
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------- 7. interfaces
def test_facade_equals_ffi(ctx):
    from options_model_amd import price_barrier_bounds

    kw = dict(n_lower=1400, n_outer=40, n_inner=64)
    for model, m in (("GBM", "gbm"), ("Heston", "heston1")):
        f = price_barrier_bounds(100.0, K, R, SIG, T, 4000, 13, 92.0, barrier_type="down-and-out", model=model,
                                 heston_params=bc.HP, heston_scheme="full_truncation", seed=42, stream=5, ctx=ctx, **kw)
        d = ctx.price_barrier_bounds(_params(m, N=13, M=4000, stream=5, hp=bc.HP), "down-and-out", 92.0, **kw)
        assert (f.lower, f.upper, f.se_lower, f.se_upper, f.inner_path_steps) == (d["lower"], d["upper"], d["se_lower"],
                                                                                  d["se_upper"], d["inner_path_steps"])
        np.testing.assert_array_equal(f.betas, d["betas"])
        assert f.policy == "textbook" and set(f.timings_ms) == {"fit", "lower", "upper", "total"}
        assert (f.barrier, f.barrier_type, f.monitoring, f.model) == (92.0, "down-and-out", "discrete", model.lower())
        assert f.lower - 4 * f.se_lower <= f.upper + 4 * f.se_upper
    s = price_barrier_bounds(100.0, K, R, SIG, T, 4000, 13, 108.0, barrier_type="up-and-in", option_type="call",
                             exercise_every=4, ctx=ctx, **kw)
    assert s.exercise_every == 4 and s.n_exercise_dates == 4 and np.count_nonzero(s.betas[:, 3]) <= 3
    k = price_barrier_bounds(100.0, K, R, SIG, T, 4000, 13, 92.0, suboptimality_check="payoff", ctx=ctx, **kw)
    assert k.suboptimality_check == "payoff" and ctx._bounds_check == 0


def test_c_example_prints_the_bounds(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "barrier_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "barrier_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    for heston, m in ((0, "gbm"), (1, "heston0")):
        out = subprocess.run([str(exe), "20", "1400", "40", "64", str(heston), "90"], check=True, capture_output=True,
                             text=True, timeout=300).stdout
        ref = ctx.price_barrier_bounds(_params(m, N=20, M=100_000, hp=bc.HP), "down-and-out", 90.0, n_lower=1400, n_outer=40,
                                       n_inner=64)
        lo, up = (float(v) for v in re.search(r"bounds \[([-0-9.]+), ([-0-9.]+)\]", out).groups())
        assert abs(lo - ref["lower"]) < 1e-6 and abs(up - ref["upper"]) < 1e-6, (out, ref)
        assert re.search(r"inner path-steps \d+", out) and "kernels:" in out and "two-pass quote" in out

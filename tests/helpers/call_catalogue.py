"""The call catalogue of the call-order tests ("call-order independence").

An omc_ctx keeps grow-only device buffers, keyed caches and options from one call to the next, and the library has no
floating-point atomics: a call's result is a function of its arguments and the options alone, bit for bit.  The
catalogue is a list of named closures `call(ctx) -> dict`, each making ONE library call (nn_build_rows: the count, then
the call with data) on device arrays of its own, and returning every numeric field of the result plus the arrays the
call wrote.  tests/test_gpu_call_order.py runs them in many orders on one context and compares each result with the
entry's result on a context of its own; tests/test_call_catalogue_cpu.py checks that every entry point is covered.

One comparison rule for all entries (`diff`): every field whose name does not start with `ms_` and is not `timed`;
floats through their bit patterns (NaN equals NaN, -0 differs from 0).

Size classes: S about 2,000 paths x 5 steps, M 20,002 x 17 (not a multiple of 4), L 140,000 x 37 (above the 65,536
paths from which the two-pass GBM pricing folds its storage by default).  Test infrastructure only: numpy and ctypes,
no torch.
"""
import contextlib
import ctypes as C
import functools
import math
from typing import Callable, NamedTuple

import numpy as np

from options_model_amd import _ffi

SIZES = {"S": (2000, 5), "M": (20002, 17), "L": (140000, 37)}
K0, R0, T0, SIG0 = 100.0, 0.05, 1.0, 0.2
HES = dict(v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7)
# the law of the QE entries (heston_scheme 3): xi = 1 violates Feller's condition, so a wave takes both branches of the scheme.
# Its constants share the cached HestonC with the Euler schemes' -- a field left over from a call at another scheme or law shows
HES_QE = dict(v0=0.04, kappa=2.0, theta=0.04, xi=1.0, rho=-0.7)
BOUNDS = dict(n_lower=4096, n_outer=64, n_inner=32, want_q=True, want_samples=True)

# every option of omc_set_option with the value a new context has (what `options` resets to)
OPTION_DEFAULTS = {"gbm_vec": 0, "heston_vec": 0, "fold_antithetic": 1, "pass2_tables": 1, "pass2_tables_irregular_every": 0,
                   "world_size": 1, "step_graph": -1, "seq_overlap": -1, "seq_event_stride": 0, "seq_step_k": -1,
                   "seq_two_pass_k": -1, "chain_fused": 0, "chain_k": -1, "seq_step_wgs": 0, "p2p_exchange": 1,
                   "p2p_deadline_ms": 2000, "p2p_first_deadline_ms": 30000, "alloc_limit": 0}


class Entry(NamedTuple):
    name: str      # family/variant/class
    family: str
    cls: str       # S, M or L
    call: Callable


CATALOGUE: list = []


# ------------------------------------------------------------------ comparison
def skipped(name):
    leaf = name.rsplit(".", 1)[-1]
    return leaf.startswith("ms_") or leaf == "timed"


def _bits(v):
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        if a.dtype.kind == "f":
            return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
        return a.astype(np.uint8) if a.dtype.kind == "b" else a.copy()
    if isinstance(v, (bool, int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return int(np.asarray(v, np.float64).view(np.uint64))
    raise TypeError(f"no bit pattern for {type(v).__name__}")


def flat(value, prefix="", out=None):
    """a result (dicts, lists, tuples, arrays, numbers, None) -> {dotted name: bit pattern}, timings dropped"""
    out = {} if out is None else out
    if isinstance(value, dict):
        for k, v in value.items():
            flat(v, f"{prefix}.{k}" if prefix else str(k), out)
    elif isinstance(value, (list, tuple)):
        if value and all(isinstance(x, (float, int, np.floating, np.integer)) and not isinstance(x, bool) for x in value):
            flat(np.asarray(value, np.float64), prefix, out)
        else:
            for i, v in enumerate(value):
                flat(v, f"{prefix}[{i}]", out)
    elif value is not None and not skipped(prefix):
        out[prefix] = _bits(value)
    return out


def diff(a, b):
    """the names of the fields in which two flat results differ (a field only one of them has differs)"""
    bad = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            bad.append(k)
        elif isinstance(a[k], np.ndarray) or isinstance(b[k], np.ndarray):
            if not (isinstance(a[k], np.ndarray) and isinstance(b[k], np.ndarray) and a[k].dtype == b[k].dtype and
                    np.array_equal(a[k], b[k])):
                bad.append(k)
        elif a[k] != b[k]:
            bad.append(k)
    return bad


@contextlib.contextmanager
def options(ctx, **opts):
    """set options for the calls inside, then put the defaults of a new context back"""
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield ctx
    finally:
        for k in opts:
            ctx.set_option(k, OPTION_DEFAULTS[k])


# ------------------------------------------------------------------ where an entry draws
class Draw(NamedTuple):
    seed: int
    stream: int
    pair_offset: int


_DRAW = None  # set by `drawing`: tests/test_gpu_rng_keys.py runs the entries at keys and counters of its choice


@contextlib.contextmanager
def drawing(seed, stream, pair_offset):
    """the entries called inside draw at this seed and pair offset and at stream + their own (small) stream, not at
    their defaults"""
    global _DRAW
    before, _DRAW = _DRAW, Draw(int(seed), int(stream), int(pair_offset))
    try:
        yield
    finally:
        _DRAW = before


def draw(seed, stream=0, pair_offset=0):
    """(seed, stream, pair_offset) of an entry: its own, unless `drawing` says otherwise"""
    if _DRAW is None:
        return seed, stream, pair_offset
    return _DRAW.seed, _DRAW.stream + stream, _DRAW.pair_offset


def run_at(name, ctx, seed, stream, pair_offset):
    """the flat result of entry `name` drawn at (seed, stream, pair_offset)"""
    with drawing(seed, stream, pair_offset):
        return flat(BY_NAME[name].call(ctx))


# ------------------------------------------------------------------ seeded host data
def P(cls, **kw):
    M, N = SIZES[cls]
    kw.setdefault("semantics", "two_pass")
    kw.setdefault("n_paths", M)
    kw.setdefault("n_steps", N)
    kw.setdefault("seed", 7 + N)
    kw.setdefault("K", K0)
    kw.setdefault("r", R0)
    kw.setdefault("T", T0)
    kw["seed"], kw["stream"], kw["pair_offset"] = draw(kw["seed"], kw.get("stream", 0), kw.get("pair_offset", 0))
    return _ffi.make_params(**kw)


@functools.lru_cache(maxsize=None)
def host_paths(cls, seed=1, S0=100.0, sigma=SIG0):
    """antithetic float32 GBM paths [N+1][M] from seeded numpy (partner of column j: j + M/2)"""
    M, N = SIZES[cls]
    z = np.random.default_rng(seed).standard_normal((N, M // 2))
    dt = T0 / N
    x = np.cumsum((R0 - 0.5 * sigma * sigma) * dt + sigma * math.sqrt(dt) * np.concatenate([z, -z], axis=1), axis=0)
    S = np.empty((N + 1, M), np.float32)
    S[0] = S0
    S[1:] = S0 * np.exp(x)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def host_normals(cls, seed):
    M, N = SIZES[cls]
    z = np.random.default_rng(seed).standard_normal((N, M // 2)).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def host_rows(n_rows, seed):
    """training rows [n][8]: 7 normalised features (the constant one 0) and the target"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_rows, 8)).astype(np.float32)
    X[:, 0] = 0.0
    X[:, 7] = 0.7 * X[:, 1] - 0.3 * X[:, 2] ** 2 + 0.1 * X[:, 7]
    X.setflags(write=False)
    return X


def mlp_param_count(hidden, layers):  # omc_mlp_param_count
    return 8 * hidden + (layers - 1) * (hidden * hidden + hidden) + hidden + 1


def localvol_param_count(layers):  # omc_localvol_param_count(64, layers)
    return 64 * 4 + layers * (64 * 64 + 3 * 64) + 65


@functools.lru_cache(maxsize=None)
def host_net(n, seed, scale=0.2):
    w = (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)
    w.setflags(write=False)
    return w


def basket3(kind="basket"):
    return _ffi.make_basket([100.0, 95.0, 105.0], [0.2, 0.3, 0.25], [0.02, 0.0, 0.01], [0.4, 0.3, 0.3] if kind == "basket"
                            else [1.0, 1.0, 1.0], [[1.0, 0.5, 0.2], [0.5, 1.0, 0.3], [0.2, 0.3, 1.0]], kind)


def state(M):
    return np.zeros(M, np.float32), np.zeros(M, np.int32)


def entry(family, variant, classes):
    """register fn(ctx, cls) once per size class as family/variant/class"""
    def deco(fn):
        for cls in classes:
            CATALOGUE.append(Entry(f"{family}/{variant}/{cls}", family, cls, functools.partial(fn, cls=cls)))
        return fn
    return deco


# ------------------------------------------------------------------ fused pricings
def _kept(ctx, cls, fn):
    """fn(keep) with a device matrix [N+1][M] of the entry's own -> its result + the matrix"""
    M, N = SIZES[cls]
    keep = ctx.to_device(np.zeros((N + 1, M), np.float32))  # (a European barrier call may leave it unwritten)
    try:
        out = fn(keep)
        out["S_keep"] = keep.to_host()
        return out
    finally:
        keep.free()


@entry("price_american", "two_pass_full", "SM")
def _(ctx, cls):
    return ctx.price_american(P(cls, sigma=SIG0))


@entry("price_american", "two_pass_folded", "L")
def _(ctx, cls):
    return ctx.price_american(P(cls, sigma=0.3, S0=95.0))


@entry("price_american", "two_pass_folded_65536", "L")
def _(ctx, cls):
    return ctx.price_american(P(cls, n_paths=65536, n_steps=5, is_put=False, S0=105.0))


@entry("price_american", "fold_forced", "SM")
def _(ctx, cls):
    with options(ctx, fold_antithetic=2):
        return ctx.price_american(P(cls, sigma=0.25))


@entry("price_american", "reference", "SML")
def _(ctx, cls):
    return ctx.price_american(P(cls, semantics="reference"))


@entry("price_american", "textbook", "SM")
def _(ctx, cls):
    return ctx.price_american(P(cls, semantics="textbook", is_put=False, S0=102.0))


@entry("price_american", "plain_call", "M")
def _(ctx, cls):
    return ctx.price_american(P(cls, antithetic=False, is_put=False, n_paths=SIZES[cls][0] - 1))


@entry("price_american", "keep_paths", "SM")
def _(ctx, cls):
    return _kept(ctx, cls, lambda keep: ctx.price_american(P(cls, stream=3), keep_paths=keep))


for _scheme in (0, 1, 2, 3):
    @entry("price_american", f"heston{_scheme}", "SM")
    def _(ctx, cls, scheme=_scheme):
        return ctx.price_american(P(cls, model="heston", heston_scheme=scheme, **HES))


@entry("price_american_seq", "two_pass_group", "L")
def _(ctx, cls):
    return {"r": ctx.price_american_seq(group_run(3))}


def group_run(n, M=70000, N=17, **kw):
    """n folded two-pass pricings of one geometry and strike: what omc_price_american_seq runs as groups"""
    return [P("L", n_paths=M, n_steps=N, is_put=(i % 2 == 0), stream=i, **kw) for i in range(n)]


@entry("price_american_seq", "two_pass_mixed", "L")
def _(ctx, cls):
    ps = [P(cls, n_paths=70000, n_steps=17, is_put=bool(i & 1), S0=95.0 + 5 * i, sigma=0.2 + 0.1 * i, stream=i) for i in range(3)]
    return {"r": ctx.price_american_seq(ps)}


@entry("price_american_seq", "two_pass_small", "SM")
def _(ctx, cls):
    return {"r": ctx.price_american_seq([P(cls, S0=98.0 + i, stream=i) for i in range(3)])}


@entry("price_american_seq", "per_step", "SM")
def _(ctx, cls):
    ps = [P(cls, semantics="reference", S0=97.0 + 2 * i, sigma=0.2 + 0.05 * i, stream=i) for i in range(4)]
    return {"r": ctx.price_american_seq(ps)}


@entry("price_american_batch", "two_pass", "SM")
def _(ctx, cls):
    M = SIZES[cls][0]
    return {"r": ctx.price_american_batch([P(cls, n_paths=M // 4 * 2 - 2 * i, S0=96.0 + 2 * i, stream=i) for i in range(5)])}


@entry("price_american_batch", "reference", "S")
def _(ctx, cls):
    return {"r": ctx.price_american_batch([P(cls, semantics="reference", S0=96.0 + 2 * i, stream=i) for i in range(5)])}


@entry("price_european", "gbm", "SL")
def _(ctx, cls):
    return ctx.price_european(P(cls, sigma=0.3))


@entry("price_european", "heston", "M")
def _(ctx, cls):
    return ctx.price_european(P(cls, model="heston", **HES))


@entry("price_european", "heston3", "M")
def _(ctx, cls):
    return ctx.price_european(P(cls, model="heston", heston_scheme=3, is_put=False, **HES_QE))


@entry("price_european_batch", "gbm", "SM")
def _(ctx, cls):
    return {"r": ctx.price_european_batch([P(cls, S0=96.0 + 2 * i, stream=i, is_put=bool(i & 1)) for i in range(5)])}


for _fused in (0, 1):
    @entry("price_american_chain", f"fused{_fused}", "SML")
    def _(ctx, cls, fused=_fused):
        n = {"S": 3, "M": 5, "L": 3}[cls]
        # the fused sweeps read folded storage: forced at the sizes that do not fold by themselves
        with options(ctx, chain_fused=fused, **({"fold_antithetic": 2} if fused and cls != "L" else {})):
            res, info = ctx.price_american_chain(P(cls, n_paths=70000 if cls == "L" else SIZES[cls][0]),
                                                 [90.0 + 7 * i for i in range(n)], [bool(i % 3) for i in range(n)], want_betas=True)
        return {"r": res, "info": info}


@entry("price_american_greeks", "want_betas", "SML")
def _(ctx, cls):
    return ctx.price_american_greeks(P(cls, sigma=0.3), want_betas=True)


@entry("price_american_greeks", "given", "S")
def _(ctx, cls):
    N = SIZES[cls][1]
    b = np.zeros((N + 1, 4))
    b[1:N] = (60.0, -0.4, -0.002, 500.0)
    return ctx.price_american_greeks(P(cls), betas=b)


for _mon in ("discrete", "continuous"):
    for _am in (True, False):
        @entry("price_barrier", f"{_mon}_{'american' if _am else 'european'}", "SM")
        def _(ctx, cls, mon=_mon, am=_am):
            kind, H = ("down-and-out", 85.0) if am else ("up-and-in", 115.0)
            return _kept(ctx, cls, lambda keep: ctx.price_barrier(P(cls, sigma=0.3), kind, H, mon, am, keep_paths=keep))


@entry("price_barrier", "heston3_discrete_american", "SM")
def _(ctx, cls):
    p = P(cls, model="heston", heston_scheme=3, **HES_QE)
    return _kept(ctx, cls, lambda keep: ctx.price_barrier(p, "down-and-out", 85.0, "discrete", True, keep_paths=keep))


@entry("price_american_div", "cash_and_yield", "SM")
def _(ctx, cls):
    return _kept(ctx, cls, lambda keep: ctx.price_american_div(P(cls), 0.01, [(0.3, 1.0), (0.7, 0.02, "proportional")], keep))


@entry("price_american_div", "heston3_cash_and_yield", "SM")
def _(ctx, cls):
    p = P(cls, model="heston", heston_scheme=3, **HES_QE)
    return _kept(ctx, cls, lambda keep: ctx.price_american_div(p, 0.01, [(0.3, 1.0), (0.7, 0.02, "proportional")], keep))


@entry("price_american_div", "yield_only", "L")
def _(ctx, cls):
    return ctx.price_american_div(P(cls), 0.03, [])


@entry("price_american_jump", "merton", "SM")
def _(ctx, cls):
    return _kept(ctx, cls, lambda keep: ctx.price_american_jump(P(cls), (1.5, -0.1, 0.15), 0.02, keep))


@entry("price_american_jump", "bates", "SM")
def _(ctx, cls):
    return ctx.price_american_jump(P(cls, model="heston", **HES), (1.0, -0.1, 0.15), 0.0)


@entry("price_american_jump", "bates3", "SM")
def _(ctx, cls):
    p = P(cls, model="heston", heston_scheme=3, **HES_QE)
    return _kept(ctx, cls, lambda keep: ctx.price_american_jump(p, (1.0, -0.1, 0.15), 0.0, keep))


@entry("price_american_basket", "basket", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    keep, akeep = ctx.to_device(np.zeros((N + 1, M), np.float32)), ctx.to_device(np.zeros((3, N + 1, M), np.float32))
    try:
        out = ctx.price_american_basket(P(cls), basket3(), keep, akeep)
        out.update(S_keep=keep.to_host(), assets=akeep.to_host())
        return out
    finally:
        keep.free()
        akeep.free()


@entry("price_american_basket", "best_of_call", "SM")
def _(ctx, cls):
    return ctx.price_american_basket(P(cls, is_put=False), basket3("best-of"))


@entry("price_american_basket_greeks", "basket", "SM")
def _(ctx, cls):
    return ctx.price_american_basket_greeks(P(cls), basket3(), want_betas=True)


@entry("price_american_basket_greeks", "worst_of_no_gamma", "S")
def _(ctx, cls):
    return ctx.price_american_basket_greeks(P(cls), basket3("worst-of"), gamma=False)


@entry("price_american_bounds", "textbook", "SM")
def _(ctx, cls):
    return ctx.price_american_bounds(P(cls), **BOUNDS)


@entry("price_american_bounds", "two_pass", "M")
def _(ctx, cls):
    return ctx.price_american_bounds(P(cls, is_put=False, S0=104.0), policy="two_pass", **BOUNDS)


@entry("price_american_bounds_heston", "textbook", "SM")
def _(ctx, cls):
    return ctx.price_american_bounds_heston(P(cls, model="heston", heston_scheme=1, **HES), **BOUNDS)


@entry("price_american_basket_bounds", "basket", "SM")
def _(ctx, cls):
    return ctx.price_american_basket_bounds(P(cls), basket3(), **BOUNDS)


@entry("price_american_basket_bounds_runnerup", "best_of", "SM")
def _(ctx, cls):
    return ctx.price_american_basket_bounds(P(cls, is_put=False), basket3("best-of"), regressors="index+runner-up", **BOUNDS)


@entry("price_american_ols7", "fused", "SML")
def _(ctx, cls):
    return ctx.price_american_ols7(P(cls))


@entry("price_american_contnet", "h32", "SM")
def _(ctx, cls):
    return ctx.price_american_contnet(P(cls, semantics="reference"), 32, 2, 1e-3, 5)


@entry("price_american_contnet_batch", "h32", "SM")
def _(ctx, cls):
    M = SIZES[cls][0] // (1 if cls == "S" else 4) // 2 * 2
    ps = [P(cls, semantics="reference", n_paths=M - 2 * i, S0=97.0 + 3 * i, stream=i) for i in range(3)]
    return {"r": ctx.price_american_contnet_batch(ps, 32, 2, 1e-3, [3, 4, 5])}


# ------------------------------------------------------------------ backward inductions on caller matrices
def _on_matrix(ctx, cls, fn, **kw):
    S = ctx.to_device(host_paths(cls, **kw))
    try:
        return fn(S)
    finally:
        S.free()


for _sem in ("reference", "textbook", "two_pass"):
    @entry("lsm_poly", _sem, "SML" if _sem == "reference" else "SM")
    def _(ctx, cls, sem=_sem):
        return _on_matrix(ctx, cls, lambda S: ctx.lsm_poly(S, K0, R0, T0, sem != "textbook", sem, want_state=True))


@entry("lsm_ols7", "state", "SM")
def _(ctx, cls):
    return _on_matrix(ctx, cls, lambda S: ctx.lsm_ols7(S, K0, R0, T0, True, want_state=True), seed=2)


@entry("lsm_contnet", "h32", "SM")
def _(ctx, cls):
    return _on_matrix(ctx, cls, lambda S: ctx.lsm_contnet(S, K0, R0, T0, True, 32, 2, 1e-3, 9), seed=3)


@entry("lsm_apply_frozen", "state", "SM")
def _(ctx, cls):
    N = SIZES[cls][1]
    b = np.zeros((N + 1, 4))
    b[1:N] = (55.0, -0.3, -0.0025, 900.0)
    return _on_matrix(ctx, cls, lambda S: ctx.lsm_apply_frozen(S, K0, R0, T0, True, b), seed=4)


@entry("lsm_apply_values", "reference", "SM")
def _(ctx, cls):
    S = host_paths(cls, seed=5)
    cont = ctx.to_device((0.9 * np.maximum(K0 - S, 0.0) + 1.0).astype(np.float32))
    try:
        return _on_matrix(ctx, cls, lambda Sd: ctx.lsm_apply_values(Sd, K0, R0, T0, True, cont), seed=5)
    finally:
        cont.free()


def _mlp_stats():
    return np.array([1.0, 1.0, 1.02, 1.06, 0.05, 0.7, 0.7]), np.array([1.0, 0.12, 0.25, 0.4, 0.06, 0.2, 0.2])


@entry("lsm_apply_mlp", "h64x2_dropout", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    S, w = ctx.to_device(host_paths(cls, seed=6)), ctx.to_device(host_net(mlp_param_count(64, 2), 21))
    fm, fs = _mlp_stats()
    res, (sx, tex) = _ffi.Result(), state(M)
    try:
        _ffi._check(ctx.lib, ctx.lib.omc_lsm_apply_mlp(ctx.handle, S.ptr, M, M, N, K0, R0, T0, 1, 64, 2, w.ptr, fm.ctypes.data,
                                                       fs.ctypes.data, 4.0, 3.0, 0.1, 123, C.byref(res), sx.ctypes.data,
                                                       tex.ctypes.data))
        return dict(res.as_dict(), sx=sx, tex=tex)
    finally:
        S.free()
        w.free()


@entry("nn_build_rows", "count_then_data", "SML")
def _(ctx, cls):
    return build_rows(ctx, host_paths(cls, seed=8), K0)


def build_rows(ctx, S_host, K, count_first=True, between=None, S_dev=None, K_count=None):
    """omc_nn_build_rows: the count call, `between(ctx, S)`, then the call with data -> n_rows, stats16 and the rows"""
    N, M = S_host.shape[0] - 1, S_host.shape[1]
    # room for the rows of either strike: a count that wrongly outlived its arguments must not write past the buffer
    cap = int(M) * max(N - 1, 1) if S_dev is not None else int((S_host[1:N] < max(K, K_count or K)).sum()) + 4096
    S = S_dev if S_dev is not None else ctx.to_device(S_host)
    data = ctx.empty((cap, 8), np.float32)  # before the count call: an allocation in between would drop what it leaves
    try:
        out = {}
        if count_first:
            out["n_count"] = ctx.nn_build_rows(S.ptr, M, M, N, K if K_count is None else K_count, R0, T0, True)
        if between is not None:
            between(ctx, S)
        n, fm, fs, ym, ys = ctx.nn_build_rows(S.ptr, M, M, N, K, R0, T0, True, data.ptr, cap)
        out.update(n_rows=n, feat_mean=fm, feat_std=fs, y_mean=ym, y_std=ys, rows=data.to_host()[:n])
        return out
    finally:
        data.free()
        if S_dev is None:
            S.free()


# ------------------------------------------------------------------ generators and taps
@entry("gbm_paths", "antithetic", "SML")
def _(ctx, cls):
    M, N = SIZES[cls]
    S = ctx.gbm_paths(M, N, 100.0, R0, 0.25, T0, *draw(11, 2, 64))
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("heston_paths", "scheme1", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    seed, stream, off = draw(12)
    S = ctx.heston_paths(M, N, 100.0, R0, T0, seed=seed, stream=stream, pair_offset=off, scheme=1, **HES)
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("heston_paths", "scheme3", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    seed, stream, off = draw(12)
    S = ctx.heston_paths(M, N, 100.0, R0, T0, seed=seed, stream=stream, pair_offset=off, scheme=3, **HES_QE)
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("heston_paths_sv", "scheme0", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    seed, stream, off = draw(13)
    S, V = ctx.heston_paths_sv(M, N, 100.0, R0, T0, seed=seed, stream=stream, pair_offset=off, scheme=0, **HES)
    try:
        return {"S": S.to_host(), "V": V.to_host()}
    finally:
        S.free()
        V.free()


@entry("gbm_paths_from_normals", "antithetic", "SM")
def _(ctx, cls):
    S = ctx.gbm_paths_from_normals(host_normals(cls, 14), 100.0, R0, 0.3, T0)
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("heston_paths_from_normals", "scheme2", "SM")
def _(ctx, cls):
    S = ctx.heston_paths_from_normals(host_normals(cls, 15), host_normals(cls, 16), 100.0, R0, T0, scheme=2, **HES)
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("gbm_normals", "tap", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    Z = ctx.gbm_normals(M // 2, N, *draw(17, 1, 32))
    try:
        return {"Z": Z.to_host()}
    finally:
        Z.free()


@entry("philox4x32_10", "tap", "SM")
def _(ctx, cls):
    n = SIZES[cls][0]
    return {"out": ctx.philox4x32_10(np.random.default_rng(18).integers(0, 2 ** 32, (n, 6), dtype=np.uint64).astype(np.uint32))}


@entry("localvol_paths", "h64", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    layers = 2 if cls == "S" else 4
    S, Z = ctx.empty((N + 1, M), np.float32), ctx.to_device(host_normals(cls, 19))
    w = ctx.to_device(host_net(localvol_param_count(layers), 20, 0.05))
    try:
        _ffi._check(ctx.lib, ctx.lib.omc_localvol_paths_f32(ctx.handle, S.ptr, M, M, N, 100.0, R0, T0, K0, 64, layers, w.ptr, 0.5,
                                                            1.0, 0.05, Z.ptr))
        return {"S": S.to_host()}
    finally:
        S.free()
        Z.free()
        w.free()


@entry("heston_price_strikes", "calibrator", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    seed, stream, _ = draw(21, 2)
    p, e = ctx.heston_price_strikes(M, N, 100.0, R0, T0, strikes=[85.0, 100.0, 110.0, 125.0], seed=seed, stream=stream, **HES)
    return {"prices": p, "stderrs": e}


@entry("heston_price_surface", "calibrator", "SM")
def _(ctx, cls):
    M, N = SIZES[cls]
    seed, stream, _ = draw(22)
    p, e = ctx.heston_price_surface(M, N, 100.0, R0, expiries=[0.25, 1.0, 2.0], streams=[stream + 1, stream + 2, stream + 3],
                                    strikes=[90.0, 100.0, 110.0, 95.0, 105.0], expiry_of=[0, 0, 1, 2, 2], is_put=True, seed=seed, **HES)
    return {"prices": p, "stderrs": e}


# ------------------------------------------------------------------ networks
def _train_bufs(ctx, hidden, layers, seed):
    n = mlp_param_count(hidden, layers)
    return ctx.to_device(host_net(n, seed)), ctx.to_device(np.zeros(n, np.float32)), ctx.to_device(np.zeros(n, np.float32))


@entry("mlp_train_epoch", "adam", "SM")
def _(ctx, cls):
    rows, batch, hidden, layers = (1000, 256, 64, 2) if cls == "S" else (20000, 4096, 128, 3)
    data = ctx.to_device(host_rows(rows, 23))
    p, m, v = _train_bufs(ctx, hidden, layers, 24)
    try:
        loss, step = ctx.mlp_train_epoch(data.ptr, rows, batch, p.ptr, m.ptr, v.ptr, 3, 1e-3, 0.1, 5, hidden=hidden,
                                         layers=layers, shuffle_key=77)
        return dict(loss=loss, step=step, params=p.to_host(), adam_m=m.to_host(), adam_v=v.to_host())
    finally:
        for a in (data, p, m, v):
            a.free()


def train_batch(ctx, n_jobs, rows, batch=256, hidden=64, layers=2, step0=0, **adam):
    """omc_mlp_train_epoch_batch on n_jobs networks of seeded rows and weights -> losses, steps and the trained buffers"""
    bufs, jobs = [], []
    try:
        for i in range(n_jobs):
            data = ctx.to_device(host_rows(rows - 16 * i, 30 + i))
            p, m, v = _train_bufs(ctx, hidden, layers, 40 + i)
            bufs += [data, p, m, v]
            jobs.append(dict(data_ptr=data.ptr, n_rows=rows - 16 * i, batch=batch, params_ptr=p.ptr, m_ptr=m.ptr, v_ptr=v.ptr,
                             step=step0 + i, lr=1e-3 * (1 + i), seed=5 + i, shuffle_key=70 + i))
        res = ctx.mlp_train_epoch_batch(jobs, hidden, layers, 0.1, **adam)
        out = {"loss": [r[0] for r in res], "step": [r[1] for r in res]}
        for i in range(n_jobs):
            out[f"net{i}"] = {k: bufs[4 * i + 1 + j].to_host() for j, k in enumerate(("params", "adam_m", "adam_v"))}
        return out
    finally:
        for a in bufs:
            a.free()


@entry("mlp_train_epoch_batch", "adam", "SM")
def _(ctx, cls):
    return train_batch(ctx, 3, 700) if cls == "S" else train_batch(ctx, 4, 6000, 1024, 128, 3)


@entry("mlp_dropout_masks", "train_and_pass2", "SM")
def _(ctx, cls):
    n = 257 if cls == "S" else 5000
    keys = np.random.default_rng(25).integers(0, 1 << 20, n).astype(np.uint32)
    return {"pass2": ctx.mlp_dropout_masks(0, 64, 2, n, 9, 77, 0.2, keys=keys), "train": ctx.mlp_dropout_masks(2, 128, 3, n, 4, 78, 0.1)}


@entry("mlp_shuffle_indices", "keyed", "SM")
def _(ctx, cls):
    n = 1001 if cls == "S" else 70001
    out = ctx.empty((n,), np.int64)
    try:
        ctx.mlp_shuffle_indices(n, 12345, out.ptr)
        return {"perm": out.to_host()}
    finally:
        out.free()


@entry("pass2_tables_check", "fits", "SM")
def _(ctx, cls):
    N = SIZES[cls][1]
    rng = np.random.default_rng(26)
    betas = np.zeros((N + 1, 4))
    betas[:, 0], betas[:, 1] = rng.normal(2.0, 3.0, N + 1), rng.normal(-50.0, 60.0, N + 1)
    betas[:, 2], betas[:, 3] = rng.normal(0.0, 300.0, N + 1), 1000.0
    mism, irr = ctx.pass2_tables_check(cls == "S", 100.0, betas, 100.0 * np.cumprod(np.full(N + 1, 1.003)), 3 if cls == "M" else 0)
    return {"mismatches": mism, "irregular": irr}


@entry("nn_feature_stats", "rows", "SM")
def _(ctx, cls):
    n, N = (3000, 5) if cls == "S" else (100001, 17)
    rng = np.random.default_rng(27)
    x, t, y = ctx.to_device(rng.uniform(0.6, 1.0, n)), ctx.to_device(rng.integers(1, N, n).astype(np.int32)), ctx.to_device(rng.uniform(0, 40, n))
    try:
        mean, var = ctx.nn_feature_stats(x.ptr, t.ptr, y.ptr, n, T0, T0 / N)
        return {"mean": mean, "var": var}
    finally:
        for a in (x, t, y):
            a.free()


@entry("contnet_init_params", "h32", "SM")
def _(ctx, cls):
    d = ctx.contnet_init_params(32 if cls == "S" else 100, SIZES[cls][1] - 1, draw(9)[0])
    return {"flat": d["flat"]}


BY_NAME = {e.name: e for e in CATALOGUE}
FAMILIES = sorted({e.family for e in CATALOGUE})


def by_class(cls):
    return [e.name for e in CATALOGUE if e.cls == cls]


# ------------------------------------------------------------------ which symbols the catalogue uses (no GPU)
class RecordingLib:
    """Stands in for libomc.so: notes the symbol of every call and reports success.  omc_alloc hands out a dummy
    address, so the closures run to their end on a machine without a GPU (their results are meaningless)."""

    def __init__(self):
        self.used = set()

    def __getattr__(self, name):
        if not name.startswith("omc_"):
            raise AttributeError(name)

        def fn(*args):
            self.used.add(name)
            if name == "omc_alloc":
                args[2]._obj.value = 4096
            return 0
        return fn


def recording_context():
    ctx = object.__new__(_ffi.Context)
    ctx.lib, ctx.handle, ctx.device, ctx._arrays, ctx._hook = RecordingLib(), C.c_void_p(1), 0, set(), None
    return ctx


def symbols_used():
    """{entry name: the omc_* symbols its closure calls}"""
    out = {}
    for e in CATALOGUE:
        ctx = recording_context()
        e.call(ctx)
        out[e.name] = set(ctx.lib.used)
        ctx.handle = None  # nothing to destroy
    return out

"""Every entry point is independent of the calls before it ("call-order independence").

An omc_ctx carries grow-only device buffers that are never cleared, keyed caches (discount table, fold tables, the
captured sweep graph, Adam bias tables, the rows cache) and a dozen options from one call to the next.  The library has
no floating-point atomics, so the criterion needs no tolerance: a call's result is a function of its arguments and the
options alone, BIT FOR BIT.  Every entry of tests/helpers/call_catalogue.py is run alone on a context of its own (the
reference, made twice: the second time after device memory was filled with 0xFF bytes and freed), then in many orders
on one context; directed sequences then aim at each named piece of state.  One process, one context at a time.
"""
import random
import time

import numpy as np
import pytest

from helpers import call_catalogue as cat
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

NAMES = [e.name for e in cat.CATALOGUE]


# ------------------------------------------------------------------ contexts and references
def dirty_device_memory():
    """about 256 MB of device arrays holding the byte 0xFF, filled and freed: best effort at handing the next context
    recycled memory that is not zero"""
    c = _ffi.Context(0)
    try:
        block = np.full(64 << 20, 0xFF, np.uint8)
        for a in [c.to_device(block) for _ in range(4)]:
            a.free()
    finally:
        c.close()


def fresh(fn, dirty=False, **opts):
    """fn on a context of its own (under `opts`) -> its flat result"""
    if dirty:
        dirty_device_memory()
    c = _ffi.Context(0)
    try:
        with cat.options(c, **opts):
            return cat.flat(fn(c))
    finally:
        c.close()


@pytest.fixture(scope="module")
def refs():
    t0 = time.perf_counter()
    out = {e.name: fresh(e.call) for e in cat.CATALOGUE}
    print(f"\n[call order] {len(out)} references on contexts of their own: {time.perf_counter() - t0:.1f} s")
    return out


def run_order(c, names, refs):
    """the entries `names` in this order on context c: every result must equal its reference"""
    fails, done = [], []
    for n in names:
        bad = cat.diff(cat.flat(cat.BY_NAME[n].call(c)), refs[n])
        if bad:
            fails.append(f"{n} after {done[-3:]}: {bad[:10]}")
        done.append(n)
    assert not fails, f"{len(fails)} results depend on the calls before them:\n" + "\n".join(fails[:25])


def on_one_context(names, refs):
    c = _ffi.Context(0)
    try:
        run_order(c, names, refs)
    finally:
        c.close()


def check_sequence(calls, **opts):
    """calls = [(label, fn)]: all of them in order on ONE context; each result must equal fn on a context of its own"""
    c = _ffi.Context(0)
    try:
        with cat.options(c, **opts):
            got = [cat.flat(fn(c)) for _, fn in calls]
    finally:
        c.close()
    fails, want = [], {}
    for i, (label, fn) in enumerate(calls):
        if label not in want:  # one label, one call
            want[label] = fresh(fn, **opts)
        bad = cat.diff(got[i], want[label])
        if bad:
            fails.append(f"{label} after {[lab for lab, _ in calls[max(i - 3, 0):i]]}: {bad[:10]}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", cat.FAMILIES)
def test_references_do_not_depend_on_what_fresh_memory_holds(refs, family):
    fails = []
    for e in cat.CATALOGUE:
        if e.family != family:
            continue
        bad = cat.diff(fresh(e.call, dirty=True), refs[e.name])
        if bad:
            fails.append(f"{e.name}: {bad[:10]}")
    assert not fails, "a first call on a new context reads memory it did not write:\n" + "\n".join(fails)


def test_entries_take_the_routes_their_names_say(ctx, refs):
    for name, folded in (("two_pass_full/S", 0), ("two_pass_full/M", 0), ("two_pass_folded/L", 1), ("two_pass_folded_65536/L", 1),
                         ("fold_forced/S", 1), ("fold_forced/M", 1), ("reference/L", 0), ("heston1/M", 0)):
        assert refs["price_american/" + name]["folded"] == folded, name
    for cls, fused in (("S", 0), ("M", 0), ("L", 0), ("S", 1), ("M", 1), ("L", 1)):
        info = refs[f"price_american_chain/fused{fused}/{cls}"]
        assert info["info.fused"] == fused and info["info.folded"] == (cls == "L" or fused == 1), (cls, fused)
    assert ctx.seq_group_width(cat.group_run(3)) == 3 and ctx.seq_group_width(cat.group_run(9, 70000, 9)) == 8
    per_step = [cat.P("M", semantics="reference", S0=97.0 + 2 * i, sigma=0.2 + 0.05 * i, stream=i) for i in range(4)]
    assert ctx.seq_step_width(per_step) == 4  # the K-per-launch sweep
    assert all(r["r[0].folded"] == 1 for r in (refs["price_american_seq/two_pass_group/L"], refs["price_american_seq/two_pass_mixed/L"]))


# ------------------------------------------------------------------ orders
def _permutation(seed):
    names = NAMES * 2
    random.Random(seed).shuffle(names)
    return names


ORDERS = {
    "catalogue": NAMES,
    "reversed": NAMES[::-1],
    "large_then_small": cat.by_class("L") + cat.by_class("S"),   # stale tails lie behind short launches
    "small_medium_large": cat.by_class("S") + cat.by_class("M") + cat.by_class("L"),  # every call is the first to need the growth
    **{f"twice_permuted_{s}": _permutation(s) for s in (1, 2, 3, 4)},
}


@pytest.mark.parametrize("order", list(ORDERS))
def test_order(refs, order):
    on_one_context(ORDERS[order], refs)


# A poison call is another family at another magnitude (S0 = K = 1e4, 41 steps, 30,002 paths, the call side): it leaves
# large non-zero values in the path matrix, the state arrays, the partials, the moment and fit tables and the sums.
def _poison_params(**kw):
    return _ffi.make_params(n_paths=30002, n_steps=41, S0=1e4, K=1e4, sigma=0.5, is_put=False, seed=99, **kw)


POISONS = [("price_american_greeks", lambda c: c.price_american_greeks(_poison_params(semantics="two_pass"), want_betas=True)),
           ("price_american_seq", lambda c: c.price_american_seq([_poison_params(semantics="reference", stream=i) for i in (0, 1)])),
           ("price_american", lambda c: c.price_american(_poison_params(semantics="two_pass")))]


@pytest.mark.parametrize("name", NAMES)
def test_entry_poison_entry(refs, name):
    e = cat.BY_NAME[name]
    c = _ffi.Context(0)
    try:
        got = [cat.flat(e.call(c))]
        for family, poison in [p for p in POISONS if p[0] != e.family][:2]:
            poison(c)
            got.append(cat.flat(e.call(c)))
    finally:
        c.close()
    for i, g in enumerate(got):
        assert not cat.diff(g, refs[name]), (name, "first call" if i == 0 else f"after poison {i}", cat.diff(g, refs[name])[:10])


def test_order_on_the_session_context(ctx, refs):
    """the first permutation on the context the rest of the suite has used"""
    run_order(ctx, ORDERS["twice_permuted_1"], refs)


# ------------------------------------------------------------------ directed sequences: one per piece of state
def _pa(**kw):
    kw.setdefault("n_paths", 2000)
    kw.setdefault("n_steps", 5)
    kw.setdefault("seed", 3)
    p = _ffi.make_params(**kw)
    return lambda c: c.price_american(p)


@pytest.mark.parametrize("semantics", ["reference", "textbook", "two_pass"])
def test_discount_table(semantics):
    """keyed by (N, r, T, address): pricings that differ only in r, only in T, only in N; N = 5 -> 300 -> 5 regrows it"""
    variants = [dict(), dict(r=0.03), dict(), dict(T=0.5), dict(r=0.03, T=0.5), dict(n_steps=6), dict(n_steps=300), dict(),
                dict(n_steps=300, r=0.03), dict(n_steps=300)]
    check_sequence([(f"price_american({semantics}, {v})", _pa(semantics=semantics, **v)) for v in variants])


def test_discount_table_under_the_other_users():
    """the European pricing, the barrier generator and the bounds read the same table"""
    def bounds(r):
        p = _ffi.make_params(semantics="two_pass", n_paths=2000, n_steps=5, r=r, seed=3)
        return lambda c: c.price_american_bounds(p, **cat.BOUNDS)

    def poly(r):
        def fn(c):
            S = c.to_device(cat.host_paths("S", seed=8))
            try:
                return c.lsm_poly(S, 100.0, r, 1.0, True, "reference")
            finally:
                S.free()
        return fn

    def european(r):
        p = _ffi.make_params(n_paths=2000, n_steps=5, r=r, seed=3)
        return lambda c: c.price_european(p)
    calls = []
    for r in (0.05, 0.02, 0.05):
        calls += [(f"bounds(r={r})", bounds(r)), (f"lsm_poly(r={r})", poly(r)), (f"price_european(r={r})", european(r)),
                  (f"price_american(r={r})", _pa(semantics="two_pass", r=r))]
    check_sequence(calls)


def test_fold_tables():
    """fold_key[2] = (N, c0, g): folded pricings that differ only in sigma (g), only in S0 (c0), only in N, interleaved
    with the sequence (both slots) and the chain (tables of its own)"""
    def one(M=70000, **v):
        return _pa(semantics="two_pass", n_paths=M, n_steps=v.pop("n_steps", 9), **v)

    def seq(**v):
        ps = cat.group_run(3, 70000, 9, **v)
        return lambda c: c.price_american_seq(ps)

    def chain(**v):
        p = _ffi.make_params(semantics="two_pass", n_paths=70000, n_steps=9, seed=3, **v)
        return lambda c: c.price_american_chain(p, [90.0, 100.0, 110.0], [True, False, True])[0]
    calls = [("base", one()), ("sigma", one(sigma=0.3)), ("base", one()), ("S0", one(S0=90.0)), ("N", one(n_steps=10)),
             ("seq base", seq()), ("sigma", one(sigma=0.3)), ("seq sigma", seq(sigma=0.3)), ("seq base", seq()), ("base", one()),
             ("chain base", chain()), ("chain sigma", chain(sigma=0.3)), ("S0", one(S0=90.0)), ("seq S0", seq(S0=90.0)),
             ("chain base", chain()), ("sigma", one(sigma=0.3)), ("r", one(r=0.01)), ("T", one(T=2.0)), ("base", one())]
    check_sequence(calls)
    check_sequence([("small " + lab, one(M=4000, **v)) for lab, v in (("base", {}), ("sigma", dict(sigma=0.3)), ("base", {}),
                                                                     ("S0", dict(S0=90.0)), ("N", dict(n_steps=10)))], fold_antithetic=2)


def test_sweep_graph():
    """option step_graph = 1, keyed by (M, N, semantics, vec4, ld, argument address): the same geometry before and after
    a larger call has regrown sx / tex / ex; lsm_poly on two caller matrices of one shape at two addresses, and on one
    matrix read at two leading dimensions"""
    M, N = 4000, 6
    big = _pa(semantics="reference", n_paths=40000, n_steps=7)
    calls = []
    for sem in ("reference", "textbook"):
        calls += [(f"{sem} small", _pa(semantics=sem, n_paths=M, n_steps=N)), ("larger", big),
                  (f"{sem} small", _pa(semantics=sem, n_paths=M, n_steps=N)), (f"{sem} K=90", _pa(semantics=sem, n_paths=M, n_steps=N, K=90.0))]
    check_sequence(calls, step_graph=1)

    rng = np.random.default_rng(5)
    A = (100.0 * np.exp(np.cumsum(rng.normal(0.0, 0.1, (N + 1, M + 64)), axis=0))).astype(np.float32)
    B = (100.0 * np.exp(np.cumsum(rng.normal(0.0, 0.12, (N + 1, M + 64)), axis=0))).astype(np.float32)

    def poly(c, S, ld):
        return c.lsm_poly(S, 100.0, 0.05, 1.0, True, "reference", want_state=True, n_paths=M) if ld == M + 64 else \
            c.lsm_poly(_View(S.ptr, (N + 1, M)), 100.0, 0.05, 1.0, True, "reference", want_state=True)

    def two_matrices(c):
        a, b = c.to_device(A), c.to_device(B)  # both live: two addresses
        try:
            return [poly(c, a, M + 64), poly(c, b, M + 64), poly(c, a, M), poly(c, a, M + 64), poly(c, b, M), poly(c, b, M + 64)]
        finally:
            a.free()
            b.free()

    def alone(S, ld):
        def fn(c):
            d = c.to_device(S)
            try:
                return poly(c, d, ld)
            finally:
                d.free()
        return fn
    want = [fresh(alone(S, ld), step_graph=1) for S, ld in ((A, M + 64), (B, M + 64), (A, M), (A, M + 64), (B, M), (B, M + 64))]
    c = _ffi.Context(0)
    try:
        with cat.options(c, step_graph=1):
            got = two_matrices(c)
    finally:
        c.close()
    for i, (g, w) in enumerate(zip(got, want)):
        assert not cat.diff(cat.flat(g), w), (i, cat.diff(cat.flat(g), w))
    assert cat.diff(want[0], want[2]) and cat.diff(want[0], want[1])  # the cases do differ


class _View(_ffi.DeviceArray):
    """the first rows x cols floats of a device array read as a matrix of another leading dimension (owns nothing)"""

    def __init__(self, ptr, shape):
        self.ptr, self.shape, self.dtype = ptr, shape, np.dtype(np.float32)


def test_rows_cache():
    """what the count call of omc_nn_build_rows leaves for the call with data: every data call returns the rows, n_rows
    and stats16 of a context of its own's count + data on the arguments of the DATA call"""
    A, B = cat.host_paths("M", seed=8), cat.host_paths("M", seed=9)
    want = {(m, K): fresh(lambda c, S=S, K=K: cat.build_rows(c, S, K)) for m, S in (("A", A), ("B", B)) for K in (100.0, 95.0)}

    def same(got, key):
        g = {k: v for k, v in cat.flat(got).items() if k != "n_count"}
        w = {k: v for k, v in want[key].items() if k != "n_count"}
        assert not cat.diff(g, w), (key, cat.diff(g, w))
    assert cat.diff(want["A", 100.0], want["B", 100.0]) and cat.diff(want["A", 100.0], want["A", 95.0])

    def other_call(c, S):
        c.price_american(cat.P("S"))

    def other_contents(c, S):
        _ffi._check(c.lib, c.lib.omc_memcpy_h2d(c.handle, S.ptr, np.ascontiguousarray(B).ctypes.data, B.nbytes))

    def option(c, S):
        c.set_option("pass2_tables", 0)
        c.set_option("pass2_tables", 1)
    c = _ffi.Context(0)
    try:
        same(cat.build_rows(c, A, 100.0), ("A", 100.0))                                  # count -> data
        same(cat.build_rows(c, A, 100.0, between=other_call), ("A", 100.0))              # count -> any other call -> data
        same(cat.build_rows(c, A, 95.0, K_count=100.0), ("A", 95.0))                     # count (K1) -> data (K2)
        same(cat.build_rows(c, A, 100.0, between=other_contents), ("B", 100.0))          # count -> other contents -> data
        same(cat.build_rows(c, A, 100.0, between=option), ("A", 100.0))                  # count -> omc_set_option -> data
        same(cat.build_rows(c, B, 100.0, count_first=False), ("B", 100.0))               # data alone, after all of that
        a, b = c.to_device(A), c.to_device(B)                                            # count on A -> data on B, one shape
        try:
            M, N = cat.SIZES["M"]
            c.nn_build_rows(a.ptr, M, M, N, 100.0, cat.R0, cat.T0, True)
            same(cat.build_rows(c, B, 100.0, count_first=False, S_dev=b), ("B", 100.0))
            same(cat.build_rows(c, A, 95.0, count_first=False, S_dev=a), ("A", 95.0))
        finally:
            a.free()
            b.free()
    finally:
        c.close()


def test_adam_bias_tables():
    """keyed by (beta1, beta2, capacity): betas (0.9, 0.999) -> (0.8, 0.99) -> (0.9, 0.999), then a job whose step
    count lies beyond the table of the earlier ones"""
    def job(step0=0, **adam):
        return lambda c: cat.train_batch(c, 2, 600, step0=step0, **adam)
    check_sequence([("default betas", job()), ("betas (0.8, 0.99)", job(beta1=0.8, beta2=0.99)), ("default betas", job()),
                    ("step 5000", job(step0=5000)), ("betas (0.8, 0.99) step 9000", job(step0=9000, beta1=0.8, beta2=0.99)),
                    ("default betas", job())])


def _larger_poly(c):
    S = c.gbm_paths(30002, 41, 1e4, 0.05, 0.5, 1.0, 5)
    try:
        return c.lsm_poly(S, 1e4, 0.05, 1.0, False, "textbook")
    finally:
        S.free()


def test_returned_tables_after_a_larger_call(refs):
    """every call that hands back `betas`, run after calls with a larger N: all rows, rows 0 and N included, equal"""
    with_betas = [n for n in NAMES if any(k.endswith("betas") or k.endswith("nitm") for k in refs[n])]
    assert len({cat.BY_NAME[n].family for n in with_betas}) >= 8, with_betas
    larger = [("greeks N=41", POISONS[0][1]), ("per-step N=41", POISONS[1][1]),
              ("chain N=41", lambda c: c.price_american_chain(_poison_params(semantics="two_pass"), [9e3, 1e4, 1.1e4], False, want_betas=True)),
              ("bounds N=41", lambda c: c.price_american_bounds(_poison_params(semantics="two_pass"), **cat.BOUNDS)),
              ("lsm_poly N=41", _larger_poly)]
    c = _ffi.Context(0)
    try:
        for _, fn in larger:
            fn(c)
        run_order(c, with_betas, refs)
        for _, fn in larger[::-1]:
            fn(c)
        run_order(c, with_betas[::-1], refs)
    finally:
        c.close()


def test_groups():
    """2 -> 9 -> 2 grouped pricings (9 exceeds the default group width of 8), a chain of 3 -> 40 -> 3 strikes, and
    seq_event_stride set and reset"""
    def seq(n, stride=0):
        ps = cat.group_run(n, 70000, 9)

        def fn(c):
            with cat.options(c, seq_event_stride=stride):
                return c.price_american_seq(ps)
        return fn

    def chain(n, fused):
        p = _ffi.make_params(semantics="two_pass", n_paths=70000 if fused else 20002, n_steps=9, seed=3)  # fused: folded

        def fn(c):
            with cat.options(c, chain_fused=fused):
                res, info = c.price_american_chain(p, [80.0 + i for i in range(n)], [bool(i & 1) for i in range(n)], want_betas=True)
            assert info["fused"] == fused
            return res
        return fn
    check_sequence([("seq 2", seq(2)), ("seq 9", seq(9)), ("seq 2", seq(2)), ("seq 9 stride 2", seq(9, 2)), ("seq 9", seq(9)),
                    ("seq 2 stride 1", seq(2, 1)), ("seq 2", seq(2))])
    for fused in (0, 1):
        check_sequence([(f"chain {n} fused {fused}", chain(n, fused)) for n in (3, 40, 3)])


# option, a value a new context does not have, and entries it reaches
OPTION_CASES = [
    ("gbm_vec", 1, ["price_american/two_pass_full/M", "price_american_div/cash_and_yield/S", "gbm_paths/antithetic/M"]),
    ("heston_vec", 1, ["price_american/heston1/M", "heston_paths/scheme1/S"]),
    ("fold_antithetic", 0, ["price_american/two_pass_folded/L", "price_american_seq/two_pass_group/L"]),
    ("fold_antithetic", 2, ["price_american/two_pass_full/M", "price_american_batch/two_pass/S"]),
    ("pass2_tables", 0, ["price_american/two_pass_full/M", "price_american_seq/two_pass_group/L", "price_american_jump/merton/S"]),
    ("pass2_tables_irregular_every", 3, ["price_american/two_pass_folded_65536/L", "price_american_bounds/textbook/S"]),
    ("world_size", 2, ["price_american/two_pass_full/M", "price_american_ols7/fused/S"]),
    ("step_graph", 1, ["price_american/reference/M", "lsm_poly/textbook/M", "lsm_apply_values/reference/S"]),
    ("seq_overlap", 1, ["price_american_seq/two_pass_group/L"]),
    ("seq_event_stride", 2, ["price_american_seq/two_pass_group/L", "price_american_seq/per_step/M"]),
    ("seq_step_k", 2, ["price_american_seq/per_step/M"]),
    ("seq_step_k", 1, ["price_american_seq/per_step/S"]),
    ("seq_two_pass_k", 2, ["price_american_seq/two_pass_group/L"]),
    ("seq_two_pass_k", 1, ["price_american_seq/two_pass_group/L"]),
    ("chain_k", 2, ["price_american_chain/fused1/M"]),
    ("seq_step_wgs", 64, ["price_american_seq/per_step/M"]),
    ("p2p_exchange", 0, ["price_american/reference/S"]),
    ("p2p_deadline_ms", 500, ["price_american/reference/S"]),
    ("p2p_first_deadline_ms", 500, ["price_american/reference/S"]),
]


def test_every_option_is_listed():
    # chain_fused belongs to the chain entries themselves; alloc_limit to test_failures
    assert {o for o, _, _ in OPTION_CASES} | {"chain_fused", "alloc_limit"} == set(cat.OPTION_DEFAULTS)


@pytest.mark.parametrize("option,value", [(o, v) for o, v, _ in OPTION_CASES])
def test_options(refs, option, value):
    """an entry under a non-default option equals a context of its own under that option; after the reset the next run
    of every affected entry equals the default reference"""
    names = next(n for o, v, n in OPTION_CASES if (o, v) == (option, value))
    c = _ffi.Context(0)
    try:
        run_order(c, names, refs)
        with cat.options(c, **{option: value}):
            under = [cat.flat(cat.BY_NAME[n].call(c)) for n in names]
        run_order(c, names, refs)
        for n, got in zip(names, under):
            want = fresh(cat.BY_NAME[n].call, **{option: value})
            assert not cat.diff(got, want), (n, option, value, cat.diff(got, want)[:10])
    finally:
        c.close()


HOOKED = ["price_american/two_pass_full/M", "price_american/reference/S", "price_american_seq/two_pass_small/S",
          "price_american_seq/per_step/S", "price_american_ols7/fused/M", "nn_build_rows/count_then_data/M"]


def test_allreduce_hook_set_and_removed(refs):
    """an identity hook (world 1) routes the sums through device memory and the collectives' scratch; once it is removed
    the same entries equal their references"""
    c = _ffi.Context(0)
    try:
        c.set_allreduce_hook(lambda dptr, count: None)
        for n in HOOKED:
            cat.BY_NAME[n].call(c)
        c.set_allreduce_hook(None)
        run_order(c, HOOKED, refs)
    finally:
        c.close()


def _refusals():
    """one refusal per family, as its own tests list them -> (raises, the entry whose next call must equal its reference)"""
    P, b3, bad = cat.P, cat.basket3, _ffi.make_basket([100.0, -1.0], [0.2, 0.2])
    return [
        (lambda c: c.price_american(P("S", n_paths=2001)), "price_american/two_pass_full/S"),
        (lambda c: c.price_european(P("S", sigma=-1.0)), "price_european/gbm/S"),
        (lambda c: c.price_american_greeks(P("S"), bump=0.0), "price_american_greeks/want_betas/S"),
        (lambda c: c.price_barrier(P("S"), "down-and-out", 120.0), "price_barrier/discrete_american/S"),
        (lambda c: c.price_american_div(P("S"), 0.0, [(0.0, 1.0)]), "price_american_div/cash_and_yield/S"),
        (lambda c: c.price_american_jump(P("S"), (-1.0, 0.0, 0.0), 0.0), "price_american_jump/merton/S"),
        (lambda c: c.price_american_basket(P("S"), bad), "price_american_basket/basket/S"),
        (lambda c: c.price_american_basket_greeks(P("S", model="heston"), b3()), "price_american_basket_greeks/basket/S"),
        (lambda c: c.price_american_bounds(P("S"), n_lower=4095, n_outer=64, n_inner=32), "price_american_bounds/textbook/S"),
        (lambda c: c.price_american_bounds_heston(P("S"), **cat.BOUNDS), "price_american_bounds_heston/textbook/S"),
        (lambda c: c.price_american_basket_bounds(P("S"), bad, **cat.BOUNDS), "price_american_basket_bounds/basket/S"),
        (lambda c: c.price_american_basket_bounds(P("S"), _ffi.make_basket([100.0, -1.0], [0.2, 0.2], kind="best-of"),
                                                  regressors="index+runner-up", **cat.BOUNDS),
         "price_american_basket_bounds_runnerup/best_of/S"),
        (lambda c: c.price_american_chain(P("S"), [100.0, -5.0]), "price_american_chain/fused0/S"),
        (lambda c: c.price_american_seq([P("S", T=-1.0)]), "price_american_seq/two_pass_small/S"),
        (lambda c: c.price_american_batch([P("S"), P("S", semantics="reference")]), "price_american_batch/two_pass/S"),
        (lambda c: c.price_american_contnet(P("S"), 32, 2), "price_american_contnet/h32/S"),
        (lambda c: c.price_american_ols7(P("S", K=0.0)), "price_american_ols7/fused/S"),
        (lambda c: c.mlp_dropout_masks(0, 64, 2, 32, 1, 1, 1.0), "mlp_dropout_masks/train_and_pass2/S"),
        (lambda c: c.heston_price_strikes(2001, 5, 100.0, 0.05, 1.0, strikes=[100.0], **cat.HES), "heston_price_strikes/calibrator/S"),
    ]


def test_failures_leave_no_trace(refs):
    """after a refused call the next call equals its reference: the library's clean error paths, on one context"""
    c = _ffi.Context(0)
    try:
        for refused, name in _refusals():
            with pytest.raises((ValueError, _ffi.OmcError)):
                refused(c)
            run_order(c, [name], refs)
    finally:
        c.close()


@pytest.mark.parametrize("name", ["price_american/two_pass_full/M", "price_american/reference/M", "price_american_greeks/want_betas/M",
                                  "price_american_bounds/textbook/M", "price_american_seq/per_step/M", "price_american_chain/fused0/M",
                                  "nn_build_rows/count_then_data/M", "price_american_ols7/fused/M", "price_american_basket/basket/M"])
def test_allocation_refused_in_the_middle_of_a_call(refs, name):
    """option alloc_limit below the call's largest buffer, at several depths: some buffers of the call have grown, one
    was refused (OmcError), and the next call equals its reference.  The option is process-wide: reset in finally."""
    e = cat.BY_NAME[name]
    c = _ffi.Context(0)
    try:
        cat.BY_NAME["price_american/two_pass_full/S"].call(c)  # small buffers exist: a refusal comes later in the call
        refused = 0
        for limit in (40_000, 200_000, 1_000_000):
            try:
                c.set_option("alloc_limit", limit)
                e.call(c)
            except _ffi.OmcError as err:
                assert "alloc_limit" in str(err), err
                refused += 1
            finally:
                c.set_option("alloc_limit", 0)
            run_order(c, [name, "price_american/two_pass_full/S"], refs)
        assert refused >= 1, "no limit was below the call's largest buffer"
    finally:
        c.set_option("alloc_limit", 0)
        c.close()

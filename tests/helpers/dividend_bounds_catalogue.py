"""The call-catalogue entries of the dividend price bounds (include/omc_dividend_bounds.h), in the
style of tests/helpers/call_catalogue.py and built on it: named closures `call(ctx) -> dict`, each making ONE library call and
returning every numeric field of the result plus the arrays the call wrote, two size classes per family.  They draw through
call_catalogue.P / call_catalogue.draw, so `call_catalogue.drawing` moves them to the keys and counters of the key sweep.
The entry points of the extension header have a signature table of their own (_ffi.DIVIDEND_BOUNDS_SIGNATURES), and this list
is their catalogue: tests/test_dividend_bounds_cpu.py checks that it calls every symbol of that table, and
tests/test_gpu_dividend_bounds_calls.py runs it for call-order independence and through the key sweep.  TEST INFRASTRUCTURE
ONLY.
"""
import functools

from helpers import call_catalogue as cat

PATHS = "seed stream offset"  # both families draw at (seed, stream, pair_offset): tests/helpers/rng_keys.py's PATHS
DRAWING = {"dividend_paths": PATHS, "price_american_bounds_div": PATHS}
DIVS = [(0.1, 1.5), (0.45, 0.02, "proportional"), (0.45, 1.0), (0.9, 2.0, "cash")]  # (T = 1 in the catalogue's params)

CATALOGUE: list = []


def entry(family, variant, classes):
    """register fn(ctx, cls) once per size class as family/variant/class"""
    def deco(fn):
        for cls in classes:
            CATALOGUE.append(cat.Entry(f"{family}/{variant}/{cls}", family, cls, functools.partial(fn, cls=cls)))
        return fn
    return deco


@entry("dividend_paths", "gbm_offset", "SM")
def _(ctx, cls):
    S = ctx.dividend_paths(cat.P(cls, sigma=cat.SIG0, seed=14, stream=2), 0.02, DIVS, step_offset=1)
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("dividend_paths", "heston_sv", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=1, seed=15, **cat.HES)
    S, V = ctx.dividend_paths(p, 0.0, DIVS, want_v=True)
    try:
        return {"S": S.to_host(), "V": V.to_host()}
    finally:
        S.free()
        V.free()


@entry("price_american_bounds_div", "gbm", "SM")
def _(ctx, cls):
    return ctx.price_american_bounds_div(cat.P(cls, sigma=cat.SIG0), 0.02, DIVS, **cat.BOUNDS)


@entry("price_american_bounds_div", "heston", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=1, **cat.HES)
    return ctx.price_american_bounds_div(p, 0.0, DIVS, **cat.BOUNDS)


BY_NAME = {e.name: e for e in CATALOGUE}
FAMILIES = sorted({e.family for e in CATALOGUE})


def symbols_used():
    """{entry name: the omc_* symbols its closure calls}, on call_catalogue's stand-in library (no GPU)"""
    out = {}
    for e in CATALOGUE:
        ctx = cat.recording_context()
        e.call(ctx)
        out[e.name] = set(ctx.lib.used)
        ctx.handle = None  # nothing to destroy
    return out


def run_at(name, ctx, seed, stream, pair_offset):
    """the flat result of entry `name` drawn at (seed, stream, pair_offset)"""
    with cat.drawing(seed, stream, pair_offset):
        return cat.flat(BY_NAME[name].call(ctx))

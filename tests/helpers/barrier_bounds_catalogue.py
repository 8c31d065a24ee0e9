"""The call-catalogue entries of the barrier price bounds (include/omc_barrier_bounds.h), in the style
of tests/helpers/call_catalogue.py and built on it, as tests/helpers/dividend_bounds_catalogue.py is: named closures
`call(ctx) -> dict`, each making ONE library call and returning every numeric field of the result plus the arrays the call
wrote, two size classes per family.  They draw through call_catalogue.P, so `call_catalogue.drawing` moves them to the keys and
counters of the key sweep.  The entry points of the extension header have a signature table of their own
(_ffi.BARRIER_BOUNDS_SIGNATURES), and this list is their catalogue: tests/test_barrier_bounds_cpu.py checks that it calls
every symbol of that table, and tests/test_gpu_barrier_bounds_calls.py runs it for call-order independence and through the key
sweep.  TEST INFRASTRUCTURE ONLY.
"""
import functools

from helpers import call_catalogue as cat

PATHS = "seed stream offset"  # both families draw at (seed, stream, pair_offset): tests/helpers/rng_keys.py's PATHS
DRAWING = {"barrier_paths_state": PATHS, "price_american_bounds_barrier": PATHS}

CATALOGUE: list = []


def entry(family, variant, classes):
    """register fn(ctx, cls) once per size class as family/variant/class"""
    def deco(fn):
        for cls in classes:
            CATALOGUE.append(cat.Entry(f"{family}/{variant}/{cls}", family, cls, functools.partial(fn, cls=cls)))
        return fn
    return deco


def _state(ctx, p, kind, H, **kw):
    arrs = ctx.barrier_paths_state(p, kind, H, **kw)
    try:
        return {k: a.to_host() for k, a in zip(("E", "S", "V", "hit"), arrs) if a is not None}
    finally:
        for a in arrs:
            if a is not None:
                a.free()


@entry("barrier_paths_state", "gbm_down_out", "SM")
def _(ctx, cls):
    return _state(ctx, cat.P(cls, sigma=cat.SIG0, seed=14, stream=2), "down-and-out", 93.0)


@entry("barrier_paths_state", "heston_up_in_restart", "SM")
def _(ctx, cls):
    return _state(ctx, cat.P(cls, model="heston", heston_scheme=1, seed=15, **cat.HES), "up-and-in", 95.0, start_hit=True)


@entry("price_american_bounds_barrier", "gbm_down_out", "SM")
def _(ctx, cls):
    return ctx.price_barrier_bounds(cat.P(cls, sigma=cat.SIG0), "down-and-out", 93.0, **cat.BOUNDS)


@entry("price_american_bounds_barrier", "heston_up_in", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=1, is_put=False, **cat.HES)
    return ctx.price_barrier_bounds(p, "up-and-in", 106.0, **cat.BOUNDS)


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

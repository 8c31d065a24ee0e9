"""The call-catalogue entries of the jump-diffusion price bounds (include/omc_jump_bounds.h), in the
style of tests/helpers/call_catalogue.py and built on it: named closures `call(ctx) -> dict`, each making ONE library call and
returning every numeric field of the result plus the arrays the call wrote, two size classes per family.  They draw through
call_catalogue.P / call_catalogue.draw, so `call_catalogue.drawing` moves them to the keys and counters of the key sweep.
The entry points of the extension header have a signature table of their own (_ffi.JUMP_BOUNDS_SIGNATURES), and this list is
their catalogue: tests/test_jump_bounds_cpu.py checks that it calls every symbol of that table, and
tests/test_gpu_jump_bounds_calls.py runs it for call-order independence and through the key sweep.  TEST INFRASTRUCTURE ONLY.
"""
import functools

from helpers import call_catalogue as cat

PATHS = "seed stream offset"  # both families draw at (seed, stream, pair_offset): tests/helpers/rng_keys.py's PATHS
DRAWING = {"jump_paths": PATHS, "price_american_bounds_jump": PATHS}

CATALOGUE: list = []


def entry(family, variant, classes):
    """register fn(ctx, cls) once per size class as family/variant/class"""
    def deco(fn):
        for cls in classes:
            CATALOGUE.append(cat.Entry(f"{family}/{variant}/{cls}", family, cls, functools.partial(fn, cls=cls)))
        return fn
    return deco


@entry("jump_paths", "merton", "SM")
def _(ctx, cls):
    S = ctx.jump_paths(cat.P(cls, sigma=cat.SIG0, seed=14, stream=2), (1.5, -0.1, 0.15), 0.02)
    try:
        return {"S": S.to_host()}
    finally:
        S.free()


@entry("jump_paths", "bates_sv", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=1, seed=15, **cat.HES)
    S, V = ctx.jump_paths(p, (1.0, -0.1, 0.15), 0.0, want_v=True)
    try:
        return {"S": S.to_host(), "V": V.to_host()}
    finally:
        S.free()
        V.free()


@entry("price_american_bounds_jump", "merton", "SM")
def _(ctx, cls):
    return ctx.price_american_bounds_jump(cat.P(cls, sigma=cat.SIG0), (1.5, -0.1, 0.15), 0.02, **cat.BOUNDS)


@entry("price_american_bounds_jump", "bates", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=1, **cat.HES)
    return ctx.price_american_bounds_jump(p, (1.0, -0.1, 0.15), 0.0, **cat.BOUNDS)


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

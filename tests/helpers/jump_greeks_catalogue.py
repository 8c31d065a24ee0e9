"""The call-catalogue entries of the jump Greeks (include/omc_jump_greeks.h), in the style of
tests/helpers/dividend_greeks_catalogue.py and built on tests/helpers/call_catalogue.py: named closures `call(ctx) -> dict`,
each making ONE library call and returning every numeric field of the result plus the policy it wrote, two size classes per
family.  They draw through call_catalogue.P, so `call_catalogue.drawing` moves them to the keys and counters of the key
sweep.  The entry point of the extension header has a signature table of its own (_ffi.JUMP_GREEKS_SIGNATURES), and this
list is its catalogue: tests/test_jump_greeks_cpu.py checks that it calls every symbol of that table, and
tests/test_gpu_jump_greeks_calls.py runs it for call-order independence and through the key sweep.  TEST INFRASTRUCTURE
ONLY.
"""
import functools

from helpers import call_catalogue as cat

PATHS = "seed stream offset"  # the family draws at (seed, stream, pair_offset): tests/helpers/rng_keys.py's PATHS
DRAWING = {"price_american_jump_greeks": PATHS}
JUMP = (1.0, -0.1, 0.15)  # (T = 1 in the catalogue's params: lambda T / N <= 1 at any step count)

CATALOGUE: list = []


def entry(family, variant, classes):
    """register fn(ctx, cls) once per size class as family/variant/class"""
    def deco(fn):
        for cls in classes:
            CATALOGUE.append(cat.Entry(f"{family}/{variant}/{cls}", family, cls, functools.partial(fn, cls=cls)))
        return fn
    return deco


@entry("price_american_jump_greeks", "gbm", "SM")
def _(ctx, cls):
    return ctx.price_american_jump_greeks(cat.P(cls, sigma=cat.SIG0, S0=100.0, is_put=True), JUMP, 0.02, bump=0.01,
                                              want_betas=True)


@entry("price_american_jump_greeks", "gbm_call_sizes_zero", "SM")
def _(ctx, cls):
    return ctx.price_american_jump_greeks(cat.P(cls, sigma=cat.SIG0, S0=104.0, is_put=False, seed=16), (2.0, 0.0, 0.0), 0.03,
                                          bump=0.02, want_betas=True)


@entry("price_american_jump_greeks", "heston", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=1, S0=100.0, is_put=True, seed=17, **cat.HES)
    return ctx.price_american_jump_greeks(p, JUMP, 0.0, bump=0.01, want_betas=True)


@entry("price_american_jump_greeks", "heston_qe", "SM")
def _(ctx, cls):
    p = cat.P(cls, model="heston", heston_scheme=3, S0=100.0, is_put=True, seed=18, stream=1, **cat.HES_QE)
    return ctx.price_american_jump_greeks(p, JUMP, 0.01, bump=0.01, want_betas=True)


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

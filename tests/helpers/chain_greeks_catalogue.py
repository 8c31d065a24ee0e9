"""The call-catalogue entries of the chain's Greeks (include/omc_chain_greeks.h), in the style of
tests/helpers/jump_greeks_catalogue.py and built on tests/helpers/call_catalogue.py: named closures `call(ctx) -> dict`,
each making ONE library call and returning every numeric field of the result plus the policies it wrote, two size classes
per family.  They draw through call_catalogue.P, so `call_catalogue.drawing` moves them to the keys and counters of the key
sweep.  The entry point of the extension header has a signature table of its own (_ffi.CHAIN_GREEKS_SIGNATURES), and this
list is its catalogue: tests/test_chain_greeks_cpu.py checks that it calls every symbol of that table, and
tests/test_gpu_chain_greeks_calls.py runs it for call-order independence and through the key sweep.  TEST INFRASTRUCTURE
ONLY.
"""
import contextlib
import functools

import numpy as np

from helpers import call_catalogue as cat

PATHS = "seed stream offset"  # the family draws at (seed, stream, pair_offset): tests/helpers/rng_keys.py's PATHS
DRAWING = {"price_american_chain_greeks": PATHS}
OPTION_DEFAULTS = {"chain_greeks_k": -1, "fold_antithetic": 1}

CATALOGUE: list = []


def entry(family, variant, classes):
    """register fn(ctx, cls) once per size class as family/variant/class"""
    def deco(fn):
        for cls in classes:
            CATALOGUE.append(cat.Entry(f"{family}/{variant}/{cls}", family, cls, functools.partial(fn, cls=cls)))
        return fn
    return deco


@contextlib.contextmanager
def options(ctx, **opts):
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        yield ctx
    finally:
        for k in opts:
            ctx.set_option(k, OPTION_DEFAULTS[k])


def _chain(cls):
    """five quotes: both sides, an American, a Bermudan and a European schedule"""
    N = cat.SIZES[cls][1]
    return [90.0, 100.0, 104.0, 100.0, 97.0], [True, True, False, True, False], [0, 3, 0, N + 3, 2]


@entry("price_american_chain_greeks", "gbm", "SM")
def _(ctx, cls):
    ks, puts, every = _chain(cls)
    res, info = ctx.price_american_chain_greeks(cat.P(cls, sigma=cat.SIG0, S0=100.0), ks, puts, bump=0.01, want_betas=True,
                                                exercise_every=every)
    return {"r": res, "info": info}


@entry("price_american_chain_greeks", "gbm_folded_k1", "SM")
def _(ctx, cls):
    ks, puts, every = _chain(cls)
    with options(ctx, fold_antithetic=2, chain_greeks_k=1):
        res, info = ctx.price_american_chain_greeks(cat.P(cls, sigma=0.3, S0=102.0, seed=21), ks, puts, bump=0.02,
                                                    want_betas=True, exercise_every=every)
    return {"r": res, "info": info}


@entry("price_american_chain_greeks", "given", "SM")
def _(ctx, cls):
    ks, puts, every = _chain(cls)
    N = cat.SIZES[cls][1]
    b = np.zeros((len(ks), N + 1, 4))
    b[:, 1:N] = (60.0, -0.4, -0.002, 500.0)
    res, info = ctx.price_american_chain_greeks(cat.P(cls, sigma=cat.SIG0, S0=100.0, seed=22), ks, puts, bump=0.01, betas=b,
                                                want_betas=True, exercise_every=every)
    return {"r": res, "info": info}


@entry("price_american_chain_greeks", "heston_qe", "SM")
def _(ctx, cls):
    ks, puts, every = _chain(cls)
    p = cat.P(cls, model="heston", heston_scheme=3, S0=100.0, seed=23, stream=1, **cat.HES_QE)
    res, info = ctx.price_american_chain_greeks(p, ks, puts, bump=0.01, want_betas=True, exercise_every=every)
    return {"r": res, "info": info}


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

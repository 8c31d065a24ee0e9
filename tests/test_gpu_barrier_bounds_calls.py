"""The barrier bounds' entry points (include/omc_barrier_bounds.h) under the two sweeps every entry point of the library
gets: call-order independence (tests/test_gpu_call_order.py) and the keys and counters of their draws
(tests/test_gpu_rng_keys.py), on the entries of tests/helpers/barrier_bounds_catalogue.py.

  * each entry's result on a context of its own equals, bit for bit, its result on one context between entries of the main
    catalogue that leave the buffers, caches and options these calls share in another state -- the barrier pricing's sums, the
    bounds workspace with and without a keep list, the path matrix -- in two orders;
  * at seed 0x9E3779B97F4A7C15, stream 0xDEADBEEF, pair_offset 2^32 - 3 the result differs when the seed's high half, its low
    half or stream bit 31 is cleared, and at pair_offset + 1 and + 2^32; it is bit-identical at stream + 2^32;
  * across the carry of the pair counter's low word: the generator's 8 pairs at 2^32 - 3 have, column by column, the bits of
    single-pair calls at 2^32 - 3 + j.
"""
import numpy as np
import pytest

from helpers import barrier_bounds_case as bc
from helpers import barrier_bounds_catalogue as bcat
from helpers import call_catalogue as cat
from helpers import rng_keys as rk
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

NAMES = [e.name for e in bcat.CATALOGUE]
SMALL = [n for n in NAMES if n.endswith("/S")]
NEIGHBOURS = [n for n in cat.BY_NAME if n.startswith("price_barrier/")][:2] + [
    "price_american_bounds/textbook/S", "price_american_bounds_heston/textbook/M", "heston_paths_sv/scheme0/M",
    "price_american/two_pass_folded/L", "price_american_basket_bounds/basket/S"]
SEED, STREAM, OFF = rk.BASE


def _fresh(call):
    c = _ffi.Context(0)
    try:
        return cat.flat(call(c))
    finally:
        c.close()


@pytest.fixture(scope="module")
def refs():
    return {n: _fresh(bcat.BY_NAME[n].call) for n in NAMES}


def test_neighbours_exist():
    assert all(n in cat.BY_NAME for n in NEIGHBOURS) and any(n.startswith("price_barrier/") for n in NEIGHBOURS)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_results_do_not_depend_on_the_calls_before_them(refs, reverse):
    order = []
    for i, n in enumerate(NAMES):  # every entry twice: after a neighbour, and directly after another entry of this list
        order += [("main", NEIGHBOURS[i % len(NEIGHBOURS)]), ("bar", n), ("bar", NAMES[(i + 3) % len(NAMES)])]
    if reverse:
        order.reverse()
    c = _ffi.Context(0)
    fails, done = [], []
    try:
        for where, n in order:
            if where == "main":
                cat.BY_NAME[n].call(c)
            else:
                bad = cat.diff(cat.flat(bcat.BY_NAME[n].call(c)), refs[n])
                if bad:
                    fails.append(f"{n} after {done[-3:]}: {bad[:10]}")
            done.append(n)
    finally:
        c.close()
    assert not fails, f"{len(fails)} results depend on the calls before them:\n" + "\n".join(fails)


def test_bounds_options_of_other_calls_are_put_back(ctx, refs):
    """a scheduled, a checked and a controlled call of the vanilla bounds through the Context methods leave the options as they
    were: the entries keep their bits"""
    p = cat.P("S", sigma=cat.SIG0)
    ctx.price_american_bounds(p, exercise_every=2, **cat.BOUNDS)
    ctx.price_american_bounds(p, suboptimality_check="european", control_variate=True, **cat.BOUNDS)
    for n in SMALL:
        assert not cat.diff(cat.flat(bcat.BY_NAME[n].call(ctx)), refs[n]), n


@pytest.mark.parametrize("name", SMALL)
def test_every_key_half_and_counter_word_changes_the_result(ctx, name):
    ref = bcat.run_at(name, ctx, *rk.BASE)
    assert ref and not cat.diff(ref, bcat.run_at(name, ctx, *rk.BASE)), name  # (and the call repeats)
    changes = rk.changes("gbm_paths")  # the PATHS list: both key halves, stream bit 31, pair_offset + 1 and + 2^32
    assert bcat.DRAWING[bcat.BY_NAME[name].family] == rk.PATHS == rk.DRAWING["gbm_paths"] and len(changes) == 5
    for what, triple in changes.items():
        assert cat.diff(ref, bcat.run_at(name, ctx, *triple)), f"{name}: same result with the {what}"
    assert cat.diff(ref, bcat.run_at(name, ctx, SEED, STREAM + (1 << 32), OFF)) == []  # only the stream's low 32 bits


@pytest.mark.parametrize("model", bc.MODELS)
def test_generator_crosses_the_carry_of_the_pair_counter(ctx, model):
    N = 9
    p = bc.with_(bc.make_params(model, N=N, M=16, seed=SEED, stream=STREAM & 0xFFFFFFFF), pair_offset=OFF)

    def paths(pp):
        return [bc.host(a) for a in ctx.barrier_paths_state(pp, "down-and-in", 96.0) if a is not None]

    whole = paths(p)
    for j in range(8):
        one = paths(bc.with_(p, n_paths=2, pair_offset=OFF + j))
        for W, O in zip(whole, one):
            W = W[:, [j, j + 8]] if W.ndim == 2 else W[[j, j + 8]]
            np.testing.assert_array_equal(W.view(np.uint32), O.view(np.uint32), err_msg=f"pair {j}")

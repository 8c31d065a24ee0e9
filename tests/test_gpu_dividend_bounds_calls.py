"""The dividend bounds' entry points (include/omc_dividend_bounds.h) under the two sweeps every entry point of the library
gets: call-order independence (tests/test_gpu_call_order.py) and the keys and counters of their draws
(tests/test_gpu_rng_keys.py), on the entries of tests/helpers/dividend_bounds_catalogue.py.

  * each entry's result on a context of its own equals, bit for bit, its result on one context between entries of the main
    catalogue that leave the buffers, caches and options these calls share in another state -- the context's dividend table
    among them, which omc_price_american_div fills with another schedule -- in two orders;
  * at seed 0x9E3779B97F4A7C15, stream 0xDEADBEEF, pair_offset 2^32 - 3 the result differs when the seed's high half, its low
    half or stream bit 31 is cleared, and at pair_offset + 1 and + 2^32; it is bit-identical at stream + 2^32;
  * across the carry of the pair counter's low word: the generator's 8 pairs at 2^32 - 3 have, column by column, the bits of
    single-pair calls at 2^32 - 3 + j.
"""
import numpy as np
import pytest

from helpers import call_catalogue as cat
from helpers import dividend_bounds_case as dc
from helpers import dividend_bounds_catalogue as dcat
from helpers import rng_keys as rk
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

NAMES = [e.name for e in dcat.CATALOGUE]
SMALL = [n for n in NAMES if n.endswith("/S")]
# entries of the main catalogue that share state with these calls: the dividend table, the path matrix, the bounds
# workspace, the discount and Heston constant caches, the exercise tables, the bounds options' neighbours
NEIGHBOURS = [n for n in cat.BY_NAME if n.startswith("price_american_div/")][:2] + [
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
    return {n: _fresh(dcat.BY_NAME[n].call) for n in NAMES}


def test_neighbours_exist():
    assert all(n in cat.BY_NAME for n in NEIGHBOURS) and any(n.startswith("price_american_div/") for n in NEIGHBOURS)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_results_do_not_depend_on_the_calls_before_them(refs, reverse):
    order = []
    for i, n in enumerate(NAMES):  # every entry twice: after a neighbour, and directly after another entry of this list
        order += [("main", NEIGHBOURS[i % len(NEIGHBOURS)]), ("div", n), ("div", NAMES[(i + 3) % len(NAMES)])]
    if reverse:
        order.reverse()
    c = _ffi.Context(0)
    fails, done = [], []
    try:
        for where, n in order:
            if where == "main":
                cat.BY_NAME[n].call(c)
            else:
                bad = cat.diff(cat.flat(dcat.BY_NAME[n].call(c)), refs[n])
                if bad:
                    fails.append(f"{n} after {done[-3:]}: {bad[:10]}")
            done.append(n)
    finally:
        c.close()
    assert not fails, f"{len(fails)} results depend on the calls before them:\n" + "\n".join(fails)


def test_bounds_options_of_other_calls_are_put_back(ctx, refs):
    """a scheduled, a checked and a controlled call of the dividend-free bounds through the Context methods leave the options
    as they were: the entries keep their bits"""
    p = cat.P("S", sigma=cat.SIG0)
    ctx.price_american_bounds(p, exercise_every=2, **cat.BOUNDS)
    ctx.price_american_bounds(p, suboptimality_check="european", control_variate=True, **cat.BOUNDS)
    for n in SMALL:
        assert not cat.diff(cat.flat(dcat.BY_NAME[n].call(ctx)), refs[n]), n


@pytest.mark.parametrize("name", SMALL)
def test_every_key_half_and_counter_word_changes_the_result(ctx, name):
    ref = dcat.run_at(name, ctx, *rk.BASE)
    assert ref and not cat.diff(ref, dcat.run_at(name, ctx, *rk.BASE)), name  # (and the call repeats)
    changes = rk.changes("gbm_paths")  # the PATHS list: both key halves, stream bit 31, pair_offset + 1 and + 2^32
    assert dcat.DRAWING[dcat.BY_NAME[name].family] == rk.PATHS == rk.DRAWING["gbm_paths"] and len(changes) == 5
    for what, triple in changes.items():
        assert cat.diff(ref, dcat.run_at(name, ctx, *triple)), f"{name}: same result with the {what}"
    assert cat.diff(ref, dcat.run_at(name, ctx, SEED, STREAM + (1 << 32), OFF)) == []  # only the stream's low 32 bits


@pytest.mark.parametrize("model", dc.MODELS)
def test_generator_crosses_the_carry_of_the_pair_counter(ctx, model):
    N, q = 9, 0.02
    divs = dc.dividends_at([(1, 1.5, "cash"), (5, 0.02, "proportional"), (9, 2.0, "cash")], 1.0, N)
    p = dc.with_(dc.make_params(model, N=N, M=16, seed=SEED, stream=STREAM & 0xFFFFFFFF), pair_offset=OFF)
    want_v = dc.is_heston(p)

    def paths(pp):
        out = ctx.dividend_paths(pp, q, divs, step_offset=2, want_v=want_v)
        return [dc.host(a) for a in (out if want_v else (out,))]

    whole = paths(p)
    for j in range(8):
        one = paths(dc.with_(p, n_paths=2, pair_offset=OFF + j))
        for W, O in zip(whole, one):
            np.testing.assert_array_equal(W[:, [j, j + 8]].view(np.uint32), O.view(np.uint32), err_msg=f"pair {j}")

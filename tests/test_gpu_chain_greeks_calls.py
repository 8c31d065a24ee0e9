"""omc_price_american_chain_greeks (include/omc_chain_greeks.h) under the two sweeps every entry point of the library gets:
call-order independence (tests/test_gpu_call_order.py) and the keys and counters of its draws
(tests/test_gpu_rng_keys.py), on the entries of tests/helpers/chain_greeks_catalogue.py.

  * each entry's result on a context of its own equals, bit for bit, its result on one context between entries of the main
    catalogue that leave the buffers this call shares in another state -- the group state and the fold and schedule tables of
    the chain, the path matrix, the discount table, the single call's Greeks partials -- in two orders;
  * at seed 0x9E3779B97F4A7C15, stream 0xDEADBEEF, pair_offset 2^32 - 3 the result differs when the seed's high half, its low
    half or stream bit 31 is cleared, and at pair_offset + 1 and + 2^32; it is bit-identical at stream + 2^32.
"""
import pytest

from helpers import call_catalogue as cat
from helpers import chain_greeks_catalogue as gcat
from helpers import rng_keys as rk
from options_model_amd import _ffi

pytestmark = pytest.mark.gpu

NAMES = [e.name for e in gcat.CATALOGUE]
SMALL = [n for n in NAMES if n.endswith("/S")]
NEIGHBOURS = [n for n in cat.BY_NAME if n.startswith("price_american_chain/")][:3] + \
             [n for n in cat.BY_NAME if n.startswith("price_american_greeks/")][:2] + ["price_american/two_pass_folded/L"]
SEED, STREAM, OFF = rk.BASE


def _fresh(call):
    c = _ffi.Context(0)
    try:
        return cat.flat(call(c))
    finally:
        c.close()


@pytest.fixture(scope="module")
def refs():
    return {n: _fresh(gcat.BY_NAME[n].call) for n in NAMES}


def test_neighbours_exist():
    assert all(n in cat.BY_NAME for n in NEIGHBOURS)
    assert any(n.startswith("price_american_chain/") for n in NEIGHBOURS)
    assert any(n.startswith("price_american_greeks/") for n in NEIGHBOURS)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_results_do_not_depend_on_the_calls_before_them(refs, reverse):
    order = []
    for i, n in enumerate(NAMES):  # every entry twice: after a neighbour, and directly after another entry of this list
        order += [("main", NEIGHBOURS[i % len(NEIGHBOURS)]), ("own", n), ("own", NAMES[(i + 3) % len(NAMES)])]
    if reverse:
        order.reverse()
    c = _ffi.Context(0)
    fails, done = [], []
    try:
        for where, n in order:
            if where == "main":
                cat.BY_NAME[n].call(c)
            else:
                bad = cat.diff(cat.flat(gcat.BY_NAME[n].call(c)), refs[n])
                if bad:
                    fails.append(f"{n} after {done[-3:]}: {bad[:10]}")
            done.append(n)
    finally:
        c.close()
    assert not fails, f"{len(fails)} results depend on the calls before them:\n" + "\n".join(fails)


@pytest.mark.parametrize("name", SMALL)
def test_every_key_half_and_counter_word_changes_the_result(ctx, name):
    ref = gcat.run_at(name, ctx, *rk.BASE)
    assert ref and not cat.diff(ref, gcat.run_at(name, ctx, *rk.BASE)), name  # (and the call repeats)
    changes = rk.changes("gbm_paths")  # the PATHS list: both key halves, stream bit 31, pair_offset + 1 and + 2^32
    assert gcat.DRAWING[gcat.BY_NAME[name].family] == rk.PATHS == rk.DRAWING["gbm_paths"] and len(changes) == 5
    for what, triple in changes.items():
        assert cat.diff(ref, gcat.run_at(name, ctx, *triple)), f"{name}: same result with the {what}"
    assert cat.diff(ref, gcat.run_at(name, ctx, SEED, STREAM + (1 << 32), OFF)) == []  # only the stream's low 32 bits

"""The call catalogue (tests/helpers/call_catalogue.py) covers the library: every symbol of _ffi.SIGNATURES is called by
an entry or excluded below for one of three reasons.  A new entry point that is in neither list fails here, which is
how it is made to join the call-order tests (tests/test_gpu_call_order.py).  No GPU: the closures run against a
stand-in library that only notes which symbols they call."""
import fnmatch

import pytest

from helpers import call_catalogue as cat
from options_model_amd import _ffi

LIFE_CYCLE = "context life cycle and raw memory helpers"
HOST = "pure host function"
SECOND_RANK = "needs a second rank"

EXCLUDED = {
    "omc_ctx_create": LIFE_CYCLE, "omc_ctx_destroy": LIFE_CYCLE, "omc_ctx_device_info": LIFE_CYCLE, "omc_alloc": LIFE_CYCLE,
    "omc_free": LIFE_CYCLE, "omc_memcpy_h2d": LIFE_CYCLE, "omc_memcpy_d2h": LIFE_CYCLE, "omc_sync": LIFE_CYCLE,
    "omc_last_error": LIFE_CYCLE, "omc_abi_version": LIFE_CYCLE, "omc_device_count": LIFE_CYCLE,
    "omc_dividend_schedule": HOST, "omc_jump_table": HOST, "omc_basket_table": HOST, "omc_mlp_param_count": HOST,
    "omc_localvol_param_count": HOST, "omc_mlp_train_supported": HOST, "omc_mlp_train_batch_supported": HOST,
    "omc_mlp_train_variant": HOST, "omc_seq_step_width": HOST, "omc_seq_group_width": HOST, "omc_chain_width": HOST,
    "omc_comm_unique_id": SECOND_RANK, "omc_comm_init": SECOND_RANK, "omc_comm_destroy": SECOND_RANK,
    "omc_comm_info": SECOND_RANK, "omc_comm_allreduce_f64": SECOND_RANK, "omc_p2p_export": SECOND_RANK,
    "omc_p2p_connect": SECOND_RANK, "omc_p2p_disconnect": SECOND_RANK, "omc_p2p_status": SECOND_RANK,
    "omc_mlp_shard_epoch": SECOND_RANK, "omc_mlp_train_epoch_sharded": SECOND_RANK, "omc_lsm_apply_mlp_shard": SECOND_RANK,
    "omc_nn_half_counts": SECOND_RANK,
}
# what each reason may name, as the patterns the design allows; omc_set_option and omc_set_allreduce_hook are not
# entries either: the directed sequences of test_gpu_call_order.py exercise them around the entries
ALLOWED = {
    LIFE_CYCLE: ["omc_ctx_*", "omc_alloc", "omc_free", "omc_memcpy_*", "omc_sync", "omc_last_error", "omc_abi_version",
                 "omc_device_count"],
    HOST: ["omc_dividend_schedule", "omc_jump_table", "omc_basket_table", "*_param_count", "*_supported", "*_variant", "*_width"],
    SECOND_RANK: ["omc_comm_*", "omc_p2p_*", "omc_mlp_shard_epoch", "omc_mlp_train_epoch_sharded", "omc_lsm_apply_mlp_shard",
                  "omc_nn_half_counts"],
}
AROUND_THE_ENTRIES = {"omc_set_option", "omc_set_allreduce_hook"}


@pytest.fixture(scope="module")
def used():
    return cat.symbols_used()


def test_every_symbol_is_called_or_excluded(used):
    called = set().union(*used.values())
    missing = sorted(set(_ffi.SIGNATURES) - called - set(EXCLUDED) - AROUND_THE_ENTRIES)
    assert not missing, f"entry points in neither the catalogue nor EXCLUDED: {missing}"
    assert not sorted(set(EXCLUDED) - set(_ffi.SIGNATURES)), "EXCLUDED names symbols the library does not have"
    # an excluded symbol that launches work through an entry after all has no business in the exclusion list
    assert not sorted((called - {"omc_alloc", "omc_free", "omc_memcpy_h2d", "omc_memcpy_d2h"}) & set(EXCLUDED))


def test_exclusions_carry_an_allowed_reason():
    for name, reason in EXCLUDED.items():
        assert reason in ALLOWED, (name, reason)
        assert any(fnmatch.fnmatchcase(name, pat) for pat in ALLOWED[reason]), f"{name} is not excluded for '{reason}'"


def test_every_entry_makes_a_call_of_its_family(used):
    for e in cat.CATALOGUE:
        work = used[e.name] - set(EXCLUDED) - AROUND_THE_ENTRIES
        assert len(work) == 1, (e.name, sorted(work))  # ONE library call per entry
        assert e.family in next(iter(work)), (e.name, work)


def test_names_are_unique_and_every_family_has_two_size_classes():
    names = [e.name for e in cat.CATALOGUE]
    assert len(names) == len(set(names))
    for fam in cat.FAMILIES:
        classes = {e.cls for e in cat.CATALOGUE if e.family == fam}
        assert len(classes) >= 2 and classes <= set(cat.SIZES), (fam, classes)
    for e in cat.CATALOGUE:
        assert e.name == f"{e.family}/{e.name.split('/')[1]}/{e.cls}"


def test_the_comparison_rule():
    import numpy as np
    a = cat.flat({"price": 1.0, "ms_total": 3.0, "timed": 1, "r": [{"x": np.nan, "ms_paths": 1.0}], "z": 0.0, "n": 3,
                  "arr": np.array([np.nan, -0.0], np.float32), "lst": [1.0, 2.0]})
    assert sorted(a) == ["arr", "lst", "n", "price", "r[0].x", "z"]
    b = cat.flat({"price": 1.0, "ms_total": 9.0, "timed": 0, "r": [{"x": np.nan, "ms_paths": 2.0}], "z": -0.0, "n": 3,
                  "arr": np.array([np.nan, 0.0], np.float32), "lst": [1.0, 2.0]})
    assert cat.diff(a, a) == [] and cat.diff(a, b) == ["arr", "z"]  # NaN equals NaN, -0 differs from 0
    assert cat.diff(a, {k: v for k, v in a.items() if k != "n"}) == ["n"]

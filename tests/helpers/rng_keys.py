"""Which catalogue families draw from the Philox counters, and at which keys and counters tests/test_gpu_rng_keys.py runs them.
TEST INFRASTRUCTURE ONLY.

Every family of tests/helpers/call_catalogue.py is in exactly one of the two lists below (tests/test_rng_keys_cpu.py): a
new entry point has to be put into one of them, so it cannot stay out of the key sweep unnoticed.
"""
from helpers import call_catalogue as cat
from helpers.rng_edges import SEED, STREAM

OFFSET = (1 << 32) - 3  # eight pairs from here cross the carry of the pair counter's low word
BASE = (SEED, STREAM, OFFSET)

PATHS = "seed stream offset"   # draws at (seed, stream, pair_offset)
NO_OFFSET = "seed stream"      # the entry point takes no pair offset
SEED_ONLY = "seed"

# family -> what its entry point takes
DRAWING = {
    "price_american": PATHS, "price_american_seq": PATHS, "price_american_batch": PATHS,
    "price_european": PATHS, "price_european_batch": PATHS,
    "price_american_chain": PATHS, "price_american_greeks": PATHS, "price_barrier": PATHS, "price_american_div": PATHS,
    "price_american_jump": PATHS,
    "price_american_basket": PATHS, "price_american_basket_greeks": PATHS,
    "price_american_bounds": PATHS, "price_american_bounds_heston": PATHS, "price_american_basket_bounds": PATHS,
    "price_american_basket_bounds_runnerup": PATHS,
    "price_american_ols7": PATHS, "price_american_contnet": PATHS, "price_american_contnet_batch": PATHS,
    "gbm_paths": PATHS, "heston_paths": PATHS, "heston_paths_sv": PATHS, "gbm_normals": PATHS,
    "heston_price_strikes": NO_OFFSET, "heston_price_surface": NO_OFFSET,
    "contnet_init_params": SEED_ONLY,
}

ON_GIVEN_DATA = "works on the caller's matrix, normals or rows: no path is drawn"
NETWORK_KEYS = "its only draws are dropout masks, shuffles or initial weights from a key of its own (tests/test_gpu_dropout.py " \
               "runs those at 64-bit seeds; the initial weights are contnet_init_params')"
NO_RANDOMNESS = "no random number at all"

DRAWS_NOTHING = {
    "lsm_poly": ON_GIVEN_DATA, "lsm_ols7": ON_GIVEN_DATA, "lsm_apply_frozen": ON_GIVEN_DATA, "lsm_apply_values": ON_GIVEN_DATA,
    "gbm_paths_from_normals": ON_GIVEN_DATA, "heston_paths_from_normals": ON_GIVEN_DATA, "localvol_paths": ON_GIVEN_DATA,
    "nn_build_rows": ON_GIVEN_DATA, "nn_feature_stats": ON_GIVEN_DATA, "philox4x32_10": ON_GIVEN_DATA,
    "lsm_contnet": NETWORK_KEYS, "lsm_apply_mlp": NETWORK_KEYS, "mlp_train_epoch": NETWORK_KEYS,
    "mlp_train_epoch_batch": NETWORK_KEYS, "mlp_dropout_masks": NETWORK_KEYS, "mlp_shuffle_indices": NETWORK_KEYS,
    "pass2_tables_check": NO_RANDOMNESS,
}


def entries():
    """the size-class-S entries of the drawing families"""
    return [e.name for e in cat.CATALOGUE if e.cls == "S" and e.family in DRAWING]


def changes(family):
    """{name: (seed, stream, pair_offset)}: each must change the result of an entry of `family`"""
    takes = DRAWING[family].split()
    out = {"seed high half cleared": (SEED & 0xFFFFFFFF, STREAM, OFFSET), "seed low half cleared": (SEED >> 32 << 32, STREAM, OFFSET)}
    if "stream" in takes:
        out["stream bit 31 cleared"] = (SEED, STREAM & 0x7FFFFFFF, OFFSET)
    if "offset" in takes:
        out["pair_offset + 1"] = (SEED, STREAM, OFFSET + 1)
        out["pair_offset + 2^32"] = (SEED, STREAM, OFFSET + (1 << 32))
    return out

"""CPU suite of the Bermudan exercise schedules of the option chain (omc_chain_entry::exercise_every):
the field travels in the chain entry's former reserved word (same offset, size, ABI number and export set), the schedule
function, the two identities the GPU tests rest on -- on the C oracle alone --, the folded restatement of
tests/helpers/bermudan_ref.py against the oracle, the facade's refusals, and the fuzz cases of tests/test_gpu_bermudan_fuzz.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from helpers import bermudan_ref as br
from oracle import cpu as orc
from options_model_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S0, K, R, SIG, T = 100.0, 100.0, 0.05, 0.2, 1.0


# ------------------------------------------------------------------ the ABI
def test_exercise_every_travels_in_the_reserved_word():
    assert [n for n, _ in _ffi.ChainEntry._fields_] == ["K", "is_put", "exercise_every"]
    assert _ffi.ChainEntry.exercise_every.offset == 12 and _ffi.ChainEntry.exercise_every.size == 4
    assert C.sizeof(_ffi.ChainEntry) == 16
    header = open(os.path.join(ROOT, "include", "omc.h")).read()
    entry = re.search(r"typedef struct \{([^}]*)\} omc_chain_entry;", header).group(1)
    assert re.search(r"int32_t\s+exercise_every;", entry) and "reserved;" not in entry
    assert re.search(r"#define OMC_ABI_VERSION\s+14\b", header)
    assert _ffi.ABI_VERSION == 14
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14
    assert not any("bermudan" in s for s in _ffi.SIGNATURES)   # no new symbol: the chain's entry point carries it
    assert len(_ffi.SIGNATURES) == 80


# ------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("N,k,dates", [
    (12, 0, list(range(1, 12))),
    (12, 1, list(range(1, 12))),
    (12, 2, [2, 4, 6, 8, 10]),
    (12, 3, [3, 6, 9]),
    (12, 11, [1]),                 # k = N - 1
    (12, 12, []),                  # k = N
    (12, 15, []),                  # k = N + 3
    (7, 3, [1, 4]),                # N % k != 0: the first date is not k
    (13, 5, [3, 8]),
    (70, 21, [7, 28, 49]),
    (252, 21, list(range(21, 252, 21))),
    (2, 2, []),
    (1, 0, []),
    (1, 5, []),
])
def test_schedule_on_hand_cases(N, k, dates):
    from options_model_amd import exercise_dates
    assert np.nonzero(br.schedule(N, k))[0].tolist() == dates
    assert exercise_dates(N, k) == dates and br.n_early(N, k) == len(dates)
    if k >= 2:
        assert len(dates) == (N - 1) // k                                     # what the library's view is sized by
        assert all((N - t) % k == 0 for t in dates) and N not in dates


# ------------------------------------------------------------------ the two identities, on the oracle
@pytest.fixture(scope="module")
def paths():
    return {N: orc.gbm_paths(4096, N, S0, R, SIG, T, seed=7) for N in (7, 12, 252)}


@pytest.mark.parametrize("is_put,strike", [(True, 100.0), (False, 95.0)])
@pytest.mark.parametrize("N,k", [(12, 3), (12, 4), (252, 21)])
def test_identity_a_masked_replay_is_the_two_pass_flow_of_the_sub_sampled_matrix(paths, N, k, is_put, strike):
    S = paths[N]
    got = br.masked_replay(S, strike, R, T, is_put, k)
    sub = orc.lsm_poly(S[::k], strike, R, T, is_put, "two_pass")
    want = sub["price"] * math.exp(-R * (T / N) * (k - 1))
    assert abs(got["price"] - want) <= 1e-13 * abs(want)
    assert got["n_exercised"] == sub["n_exercised"] and (got["n_exercised"] > 0 or not is_put)
    assert got["sum_nitm"] == sub["sum_nitm"]
    # the same regressions up to the rounding of the discount's exponent (r (T / N) (N - t) against r (k T / N) (N - t) / k)
    assert np.allclose(got["betas4"][::k][1:-1, :3], sub["betas"][1:-1], rtol=1e-9, atol=1e-12)
    assert np.array_equal(got["nitm"][::k], sub["nitm"])
    assert np.array_equal(got["tex"] // k, sub["tex"])


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("N,k", [(7, 7), (7, 9), (12, 12)])
def test_identity_b_no_early_date_is_the_european_value_of_the_flow(paths, N, k, is_put):
    S = paths[N]
    got = br.masked_replay(S, K, R, T, is_put, k)
    s, _ = orc.european_from_paths(S, K, R, T, is_put)
    want = s / S.shape[1] * math.exp(R * T / N)
    assert got["n_exercised"] == 0 and got["sum_nitm"] == 0 and not got["betas4"].any()
    assert abs(got["price"] - want) <= 1e-13 * want


# ------------------------------------------------------------------ the folded restatement
def _half(N, P=2048, seed=7):
    return orc.gbm_paths(P, N, S0, R, SIG, T, seed=seed, antithetic=0)


@pytest.mark.parametrize("is_put,strike", [(True, 100.0), (False, 97.0)])
@pytest.mark.parametrize("N", [1, 2, 7, 12, 70])
def test_folded_restatement_with_every_date_is_the_oracles_folded_flow(N, is_put, strike):
    S = _half(N)
    c0, g = orc.fold_constants(S0, strike, R, SIG, T, N)
    ref = orc.lsm_two_pass_folded(S, strike, R, T, is_put, c0, g)
    for k in (0, 1):
        got = br.folded_two_pass(S, strike, R, T, is_put, c0, g, k)
        assert got["margin"] > br.TIE
        for key in ("n_paths", "n_exercised", "n_zero", "sum_nitm"):
            assert got[key] == ref[key], key
        assert np.array_equal(got["nitm"], ref["nitm"])
        assert np.array_equal(got["texa"], ref["texa"]) and np.array_equal(got["texb"], ref["texb"])
        for key in ("price", "sum", "sumsq"):
            assert abs(got[key] - ref[key]) <= 1e-12 * abs(ref[key]), key
        assert np.allclose(got["betas4"][:, :3], ref["betas"], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("N,k", [(12, 3), (12, 5), (13, 5), (70, 21), (7, 6), (7, 7), (7, 10), (2, 2), (1, 2)])
def test_folded_restatement_with_a_mask_is_the_flow_on_the_explicit_partner_matrix(N, k, is_put):
    """The partner's moneyness is fma(cK, 1 / S, -1) in the folded flow and (cK K / S) / K - 1 on the explicit matrix: a few
    units of 1e-16 apart, which the fits may amplify; the bound is the 1e-9 of every comparison of two summation orders."""
    S = _half(N)
    c0, g = orc.fold_constants(S0, K, R, SIG, T, N)
    got = br.folded_two_pass(S, K, R, T, is_put, c0, g, k)
    ref = br.matrix_two_pass(br.partner_matrix(S, K, c0, g), K, R, T, is_put, k)
    assert min(got["margin"], ref["margin"]) > br.TIE
    ok, bad = br.agrees(got, ref)
    assert ok, bad
    assert np.array_equal(got["nitm"], ref["nitm"]) and np.array_equal(got["tex"], ref["tex"])
    mask = br.schedule(N, k)
    assert not got["nitm"][~mask].any() and not got["betas4"][~mask].any()
    assert set(np.unique(got["tex"])) <= set(np.nonzero(mask)[0]) | {N}
    assert got["sum_nitm"] == int(got["nitm"][mask].sum())
    if k >= N:
        assert got["n_exercised"] == 0 and got["sum_nitm"] == 0


def test_folded_restatement_on_the_first_half_of_the_full_matrix_tracks_the_masked_replay():
    """Float32 partners (the full matrix) against float64 ones (the fold): the 5e-6 of tests/test_gpu_fold.py."""
    N, k = 12, 3
    full = orc.gbm_paths(4096, N, S0, R, SIG, T, seed=7)
    c0, g = orc.fold_constants(S0, K, R, SIG, T, N)
    got = br.folded_two_pass(full[:, :2048], K, R, T, True, c0, g, k)
    ref = br.masked_replay(full, K, R, T, True, k)
    assert abs(got["price"] - ref["price"]) <= 5e-6 * ref["price"]
    assert abs(got["n_exercised"] - ref["n_exercised"]) <= 4


# ------------------------------------------------------------------ the facade
@pytest.mark.parametrize("kw,match", [
    (dict(exercise_every=-1), "non-negative integer"),
    (dict(exercise_every=2.5), "non-negative integer"),
    (dict(exercise_every="3"), "non-negative integer"),
    (dict(exercise_every=True), "non-negative integer"),
    (dict(exercise_every=float("nan")), "non-negative integer"),
    (dict(exercise_every=[3, -2]), "non-negative integer"),
    (dict(exercise_every=[3, 1.5]), "non-negative integer"),
    (dict(exercise_every=[3]), "one per strike"),
    (dict(exercise_every=[3, 3, 3]), "one per strike"),
    (dict(n_gpus=2), "one GPU"),
    (dict(n_gpus=0), "one GPU"),
])
def test_facade_refuses_bad_schedules_without_a_context(monkeypatch, kw, match):
    import options_model_amd

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_ffi, "default_context", no_library)
    monkeypatch.setattr(_ffi, "load_library", no_library)
    args = dict(S0=100.0, strikes=[95.0, 100.0], r=0.05, sigma=0.2, T=1.0, n_paths=10_000, n_steps=50)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        options_model_amd.price_american_chain(**args)
    if "exercise_every" in kw and not isinstance(kw["exercise_every"], list):
        one = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=10_000, n_steps=50, **kw)
        with pytest.raises(ValueError, match=match):
            options_model_amd.price_bermudan_option(**one)


def test_facade_takes_integral_schedules_of_any_integer_type(monkeypatch):
    from options_model_amd import api
    assert api._schedules(None, 3) == [0, 0, 0] and api._schedules(5, 2) == [5, 5]
    assert api._schedules(np.int64(21), 2) == [21, 21] and api._schedules(3.0, 1) == [3]
    assert api._schedules([0, np.int32(1), 63], 3) == [0, 1, 63] and api._schedules(np.array([2, 3]), 2) == [2, 3]
    with pytest.raises(ValueError):
        api.price_bermudan_option(100.0, 100.0, 0.05, 0.2, 1.0, 1000, 10, None)
    with pytest.raises(ValueError):
        api.price_bermudan_option(100.0, 100.0, 0.05, 0.2, 1.0, 1000, 10, [2])


def test_binding_sets_the_field(monkeypatch):
    e = _ffi.ChainEntry(100.0, 1, 21)
    assert (e.K, e.is_put, e.exercise_every) == (100.0, 1, 21)
    assert _ffi.ChainEntry(100.0, 1).exercise_every == 0          # every current caller: the American quote


# ------------------------------------------------------------------ the fuzz cases
@pytest.mark.parametrize("seed", [232323, 0, 1, 99])
def test_fuzz_generator_deals_what_the_sweep_is_there_for(seed):
    cases = br.fuzz_cases(24, seed)
    head = cases[:8]
    assert sum(c["folded"] for c in head) == 3 and sum(c["model"] == "heston" for c in head) == 3
    assert any(c["folded"] and (c["M"] // 2) % 4 == 0 for c in head) and any(c["folded"] and (c["M"] // 2) % 2 == 1 for c in head)
    assert any(not c["folded"] and c["M"] % 4 == 0 for c in head) and any(not c["folded"] and c["M"] % 4 != 0 for c in head)
    assert any(c["N"] % c["k"] != 0 and 2 <= c["k"] < c["N"] for c in head)
    assert any(c["k"] >= c["N"] for c in head) and any(c["k"] == c["N"] - 1 for c in head)
    assert {c["scheme"] for c in cases if c["model"] == "heston"} == {0, 1, 3}
    assert any(c["pair_offset"] for c in head)
    for c in cases:
        assert c["M"] % 2 == 0 and 2400 <= c["M"] <= 12_002 and 1 <= c["N"] <= 70 and c["k"] >= 2
        assert not (c["folded"] and c["model"] != "gbm")


@pytest.mark.parametrize("i", range(8))
def test_fuzz_case_restates_without_a_tie(i):
    c = br.fuzz_cases(8, 232323)[i]
    ref = br.reference(c, br.oracle_paths(c, half=c["folded"]))
    assert ref["margin"] > br.TIE, (c, ref["margin"])
    assert ref["n_paths"] == c["M"]
    assert ref["sum_nitm"] == int(ref["nitm"][br.schedule(c["N"], c["k"])].sum())
    if c["k"] >= c["N"]:
        assert ref["n_exercised"] == 0

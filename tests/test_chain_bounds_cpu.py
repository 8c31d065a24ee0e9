"""What omc_price_american_chain_bounds offers without a GPU: the symbol, the extension header and the
ctypes mirror of its struct; the facade's argument checks, which come before any device call; the numpy restatement of the
multi-policy inner sweep (helpers/chain_bounds_ref.py) against the single-option restatement (helpers/bounds_ref.py) entry by
entry, with the step-count relations of the contract; and the limits of the fuzz cases."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import bounds_ref as br
from helpers import chain_bounds_case as cc
from helpers import chain_bounds_catalogue as cat
from helpers import chain_bounds_ref as cr
from options_model_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_symbol_header_and_struct():
    lib = _ffi.load_library()
    name = "omc_price_american_chain_bounds"
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80  # the set omc.h declares stays that set
    assert list(_ffi.CHAIN_BOUNDS_SIGNATURES) == [name]
    others = (set(_ffi.SIGNATURES) | set(_ffi.JUMP_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_BOUNDS_SIGNATURES)
              | set(_ffi.BARRIER_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_GREEKS_SIGNATURES))
    assert name not in others
    res, args = _ffi.CHAIN_BOUNDS_SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 11 and len(getattr(lib, name).argtypes) == 11  # exported and bound
    header = open(os.path.join(ROOT, "include", "omc_chain_bounds.h")).read()
    assert '#include "omc.h"' in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(omc_[a-z0-9_]+)\s*\(", code))) == [name]
    proto = re.search(r"\bint omc_price_american_chain_bounds\((.*?)\);", code, flags=re.S).group(1)
    params = [" ".join(a.split()) for a in proto.split(",")]
    assert params == ["omc_ctx* ctx", "const omc_params* p", "const omc_chain_entry* entries", "int n_entries",
                      "const omc_bounds_config* cfg", "const double* betas", "double* betas_out", "double* q_out",
                      "double* samples_out", "omc_bounds* out", "omc_chain_bounds_info* info"]
    assert args[2]._type_ is _ffi.ChainEntry and args[4]._type_ is _ffi.BoundsConfig
    assert args[9]._type_ is _ffi.Bounds and args[10]._type_ is _ffi.ChainBoundsInfo and args[3] is ctypes.c_int
    # the info struct, field by field as the header declares it
    body = re.search(r"typedef struct \{(.*?)\} omc_chain_bounds_info;", code, flags=re.S).group(1)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    declared = []
    for stmt in body.split(";"):
        words = stmt.replace(",", " ").split()
        declared += [(w, ctype[words[0]]) for w in words[1:]]
    assert declared == list(_ffi.ChainBoundsInfo._fields_)
    assert ctypes.sizeof(_ffi.ChainBoundsInfo) == 8 + 2 * 4 + 4 * 8
    assert int(re.search(r"#define OMC_CHAIN_BOUNDS_MAX (\d+)", header).group(1)) == _ffi.CHAIN_BOUNDS_MAX == cc.CAP
    assert re.search(r"#define OMC_ABI_VERSION 14\b", open(os.path.join(ROOT, "include", "omc.h")).read())
    # the existing structs the entry point takes keep their sizes
    assert (ctypes.sizeof(_ffi.ChainEntry), ctypes.sizeof(_ffi.BoundsConfig), ctypes.sizeof(_ffi.Bounds)) == (16, 56, 120)


def test_both_sources_are_built_and_the_cap_is_the_kernels():
    from options_model_amd import _build

    assert {"omc_chain_bounds.hip", "omc_api_chain_bounds.hip"} <= set(_build.SOURCES)
    assert {"omc_chain_bounds.h", "omc_chain_bounds_dev.h"} <= set(_build.HEADERS)
    h = open(os.path.join(_build.CSRC, "omc_chain_bounds.h")).read()
    assert int(re.search(r"constexpr int kChainBoundsMax = (\d+);", h).group(1)) == _ffi.CHAIN_BOUNDS_MAX
    assert int(re.search(r"constexpr size_t kChainBoundsLds = (\d+);", h).group(1)) == 65536


# ------------------------------------------------------------------ the facade
ARGS = dict(S0=100.0, strikes=[90.0, 100.0], r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, device=10 ** 6)


@pytest.mark.parametrize("kw,match", [
    (dict(model="SABR"), "model must be"), (dict(strikes=[]), "must not be empty"), (dict(strikes=7.0), "sequence of numbers"),
    (dict(strikes=[100.0] * 257), "at most 256"), (dict(option_types=["put"]), "one per strike"),
    (dict(option_types=["put", "straddle"]), "option_type"), (dict(strikes=[100.0, -1.0]), "must be positive"),
    (dict(strikes=[100.0, float("nan")]), "must be positive"), (dict(policy="best"), "policy must be"),
    (dict(policy="given"), "betas must be given"), (dict(betas=np.zeros((2, 5, 4))), "betas must be given"),
    (dict(policy="given", betas=np.zeros((5, 4))), "betas must have shape"),
    (dict(policy="given", betas=np.zeros((3, 5, 4))), "betas must have shape"),
    (dict(n_lower=3), "n_lower"), (dict(n_outer=0), "n_outer"), (dict(n_inner=7), "n_inner"),
    (dict(model="Heston", heston_scheme="qe"), "heston_scheme 'reference' or 'full_truncation'"),
    (dict(model="Heston", heston_scheme="calibrator"), "heston_scheme 'reference' or 'full_truncation'"),
    (dict(model="Heston", heston_scheme="milstein"), "heston_scheme must be"),
    (dict(sigma=None), "sigma"), (dict(sigma=-0.2), "sigma"), (dict(T=0.0), "must be positive"), (dict(r=-0.01), "non-negative"),
    (dict(n_steps=0), "positive integers"), (dict(n_paths=1), "positive integers")],
    ids=["model", "empty", "scalar", "long", "types-short", "type", "strike-negative", "strike-nan", "policy", "given-none",
         "betas-unasked", "given-2d", "given-long", "n_lower", "n_outer", "n_inner", "qe", "calibrator", "scheme", "sigma-none",
         "sigma-negative", "T", "r", "steps", "paths"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_american_chain_bounds

    args = dict(ARGS)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_american_chain_bounds(**args)


def test_facade_reaches_the_context_only_with_valid_arguments(monkeypatch):
    from options_model_amd import ChainBoundsResult, price_american_chain_bounds

    class Reached(Exception):
        pass

    def no_context(device=None):
        assert device == 10 ** 6
        raise Reached

    monkeypatch.setattr(_ffi, "default_context", no_context)
    for kw in (dict(), dict(model="Heston", sigma=None), dict(model="Heston", heston_scheme="full_truncation"),
               dict(policy="given", betas=np.zeros((2, 5, 4))), dict(option_types=["call", "put"])):
        args = dict(ARGS)
        args.update(kw)
        with pytest.raises(Reached):
            price_american_chain_bounds(**args)
    assert issubclass(ChainBoundsResult, list)


# ------------------------------------------------------------------ the restatement
ENTRIES = [(100.0, True, "flat"), (200.0, True, "flat"), (60.0, True, "flat"), (95.0, False, "holes"), (100.0, True, "zero")]


def _entries(N):
    case = cc.make_case(N=N, policy="given", strikes=[k for k, _, _ in ENTRIES], puts=[p for _, p, _ in ENTRIES],
                        given=[g for _, _, g in ENTRIES])
    return [(k, p, t) for (k, p, _), t in zip(ENTRIES, cc.given_tables(case))]


@pytest.mark.parametrize("N,n_inner", [(5, 8), (1, 2), (7, 6)])
def test_the_multi_policy_sweep_is_the_single_sweep_entry_by_entry(N, n_inner):
    r, T = 0.05, 1.0
    So, inner = cr.numpy_gbm_case(7 + N, N=N, n_outer=4, n_inner=n_inner)
    entries = _entries(N)
    rows = range(So.shape[1])
    got = cr.q_rows(So, inner, rows, r, T, entries)
    assert got["ties"] == 0
    for e, (K, is_put, b4) in enumerate(entries):
        ref = br.q_rows(So, inner, rows, K, r, T, is_put, b4)
        assert ref["ties"] == 0
        assert got["inner_path_steps"][e] == ref["inner_path_steps"]  # every path stopped where the single sweep's did
        # (pair sums first, then the item's sum: another order than the restatement's flat sum)
        np.testing.assert_allclose(got["q"][e], ref["q"], rtol=1e-14, atol=1e-14 * K)
    steps = got["inner_path_steps"]
    assert max(steps) <= got["simulated"] <= sum(steps)
    items = So.shape[1] * n_inner
    # the all-zero table never stops before N: it alone decides how long every pair is simulated
    assert steps[-1] == items * N * (N + 1) // 2 == got["simulated"]
    if N > 1:
        assert steps[1] == items * N  # half the strike in the money against a table value of a few percent of it: stops at once
        assert min(steps) < max(steps)


def test_the_sweep_ends_with_the_last_entry_and_identical_entries_cost_one():
    N, r, T = 6, 0.05, 1.0
    So, inner = cr.numpy_gbm_case(3, N=N, n_outer=2, n_inner=8)
    flat, deep = _entries(N)[0], _entries(N)[1]
    one = cr.q_rows(So, inner, range(2), r, T, [flat])
    three = cr.q_rows(So, inner, range(2), r, T, [flat, flat, flat])
    assert three["simulated"] == one["simulated"] == one["inner_path_steps"][0] == max(three["inner_path_steps"])
    assert np.array_equal(three["q"][0], one["q"][0]) and np.array_equal(three["q"][2], one["q"][0])
    it = cr.item(inner(0, 2), 2, N, r, T, [deep])
    assert it["swept"] == 1 and it["steps"] == [8] and it["simulated"] == 8  # everyone stops at the first date: one step
    both = cr.item(inner(0, 2), 2, N, r, T, [deep, flat])
    alone = cr.item(inner(0, 2), 2, N, r, T, [flat])
    assert both["swept"] == alone["swept"] and both["simulated"] == alone["simulated"]
    assert both["steps"] == [8, alone["steps"][0]] and both["q"][1] == alone["q"][0]


# ------------------------------------------------------------------ the cases
def test_fuzz_cases_stay_inside_the_entry_points_limits():
    cases = cc.fuzz_cases(60)
    assert cases[:10] == cc.fuzz_cases(10)  # seeded
    lim = cc.LIMITS
    for c in cases:
        E = len(c["strikes"])
        assert lim["E"][0] <= E <= lim["E"][1] <= _ffi.CHAIN_MAX and len(c["puts"]) == E
        assert lim["N"][0] <= c["N"] <= lim["N"][1] and c["M"] % 2 == 0 and lim["M"][0] <= c["M"] <= lim["M"][1]
        for k in ("n_lower", "n_outer", "n_inner"):
            assert c[k] >= 2 and c[k] % 2 == 0
        assert lim["n_outer"][0] <= c["n_outer"] <= lim["n_outer"][1] and c["n_inner"] in cc.N_INNER
        assert c["n_outer"] * (c["N"] + 1) * c["n_inner"] <= 2 ** 32
        assert all(k > 0 and np.isfinite(k) for k in c["strikes"]) and c["policy"] in _ffi.BOUND_POLICIES
        assert (c["given"] is not None) == (c["policy"] == "given")
        assert c["model"] in ("gbm", "heston") and c["scheme"] in (0, 1) and -1.0 <= c["rho"] <= 1.0 and c["v0"] >= 0
        tabs = cc.given_tables(c)
        assert tabs is None or tabs.shape == (E, c["N"] + 1, 4)
    assert {c["model"] for c in cases} == {"gbm", "heston"} and {c["n_inner"] for c in cases} == set(cc.N_INNER)
    assert any(len(c["strikes"]) > cc.CAP for c in cases) and any(len(c["strikes"]) == 1 for c in cases)
    assert {c["policy"] for c in cases} == set(cc.POLICIES) and any(c["irr_every"] for c in cases)


def test_the_catalogue_covers_what_the_contract_names():
    exact, tol = cat.EXACT_CASES.values(), cat.TOLERANCE_CASES.values()
    assert {c["n_inner"] for c in exact} == {2, 64, 128} and {c["n_inner"] for c in tol} == {130, 512}
    for cases in (exact, tol):
        assert {c["model"] for c in cases} == {"gbm", "heston"}
        assert {c["N"] for c in cases} == {5, 8, 9}
        assert all(64 <= c["n_outer"] <= 256 and c["n_lower"] == 4096 and c["M"] == 8192 for c in cases)
    assert {len(c["strikes"]) for c in exact} >= {1, 2, 3, cc.CAP, cc.CAP + 1}
    assert any(len(set(c["puts"])) == 2 for c in exact) and any(c["irr_every"] for c in exact)
    assert any(c["policy"] == "given" and "zero" in c["given"] for c in exact)
    assert all(len(set(c["strikes"])) == 1 and len(c["strikes"]) >= 2 for c in cat.TWIN_CASES.values())
    assert 0.0 < 4.0 * cc.MEASURED_UPPER_REL < 1e-9 and 0.0 < 4.0 * cc.MEASURED_Q_REL < 1e-9


def test_c_example_compiles_against_the_header_and_library(tmp_path):
    import shutil
    import subprocess

    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    exe = tmp_path / "american_chain_bounds"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "american_chain_bounds.c"), "-o", str(exe), "-L", os.path.dirname(lib), "-lomc",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    assert exe.exists()

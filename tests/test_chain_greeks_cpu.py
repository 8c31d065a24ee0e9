"""What omc_price_american_chain_greeks offers without a GPU: the symbol, its table and the info
struct, the C example against the header and the library, the facades' argument checks, the catalogue on the stand-in
library, and the restatement of the kernel's route for a Bermudan entry (helpers/chain_greeks_ref.py: the view's rows, the
step map, d2 and cv) against tests/helpers/greeks_ref.py on the full matrix under the masked policy -- contract 2 of
include/omc_chain_greeks.h, in numpy -- and the fuzz cases' freedom from ties."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bermudan_ref as br
from helpers import chain_greeks_catalogue as gcat
from helpers import chain_greeks_ref as cg
from helpers import greeks_ref as gr
from oracle import cpu as orc
from options_model_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "omc_price_american_chain_greeks"
S0, R, SIG, T = 100.0, 0.05, 0.2, 1.0


# ------------------------------------------------------------------ the interface
def test_symbol_table_and_info_struct():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    assert list(_ffi.CHAIN_GREEKS_SIGNATURES) == [NAME]
    others = (set(_ffi.SIGNATURES) | set(_ffi.JUMP_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_BOUNDS_SIGNATURES)
              | set(_ffi.BARRIER_BOUNDS_SIGNATURES) | set(_ffi.DIVIDEND_GREEKS_SIGNATURES) | set(_ffi.CHAIN_BOUNDS_SIGNATURES)
              | set(_ffi.JUMP_GREEKS_SIGNATURES))
    assert NAME not in others
    assert len(_ffi.CHAIN_GREEKS_SIGNATURES[NAME][1]) == 9
    assert len(getattr(lib, NAME).argtypes) == 9  # exported and bound
    header = open(os.path.join(ROOT, "include", "omc_chain_greeks.h")).read()
    assert '#include "omc.h"' in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(omc_[a-z0-9_]+)\s*\(", code))) == [NAME]
    assert re.search(r"\bint omc_price_american_chain_greeks\(omc_ctx\* ctx, const omc_params\* p, const omc_chain_entry\* e, "
                     r"int n, double bump,\s*const double\* betas, double\* betas_out, omc_greeks\* out,\s*"
                     r"omc_chain_greeks_info\* info\);", header)
    assert re.search(r"#define OMC_ABI_VERSION 14\b", open(os.path.join(ROOT, "include", "omc.h")).read())
    # four int32 and four doubles, in the header's order
    assert ctypes.sizeof(_ffi.ChainGreeksInfo) == 4 * 4 + 4 * 8
    assert [n for n, _ in _ffi.ChainGreeksInfo._fields_] == re.findall(
        r"\b(folded|n_groups|n_sweep_launches|entries_per_launch|ms_paths|ms_pass1|ms_greeks|ms_total)[,;]",
        code.split("typedef struct {")[1].split("}")[0])


def test_c_example_compiles_against_the_header_and_the_library(tmp_path):
    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "american_chain_greeks.c"), "-o", str(tmp_path / "american_chain_greeks"),
                    "-L", os.path.dirname(lib), "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)


ARGS = dict(S0=100.0, strikes=[95.0, 100.0], r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, device=10 ** 6)


@pytest.mark.parametrize("kw,match", [
    (dict(model="SABR"), "model"), (dict(strikes=[]), "strikes"), (dict(strikes=7.0), "strikes"),
    (dict(strikes=[100.0] * 257), "at most"), (dict(option_types=["put"]), "option_types"),
    (dict(exercise_every=[1]), "exercise_every"), (dict(exercise_every=-2), "exercise_every"),
    (dict(strikes=[100.0, -1.0]), "positive"), (dict(option_types="straddle"), "option_type"),
    (dict(model="Heston", heston_scheme="milstein"), "heston_scheme"), (dict(n_steps=0), "positive"),
    (dict(bump=0.0), "bump"), (dict(bump=0.6), "bump"), (dict(bump=float("nan")), "bump"),
    (dict(betas=np.zeros((2, 4, 4))), "betas")],
    ids=["model", "empty", "not-a-sequence", "too-many", "sides", "schedules", "schedule-negative", "strike", "option-type",
         "scheme", "steps", "bump-0", "bump-large", "bump-nan", "betas-shape"])
def test_chain_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_american_chain_greeks
    with pytest.raises(ValueError, match=match):
        price_american_chain_greeks(**dict(ARGS, **kw))


def test_the_chains_own_checks_come_first_and_in_its_order():
    """a fault price_american_chain raises wins over the bump's, and it is the same fault"""
    from options_model_amd import price_american_chain, price_american_chain_greeks
    for kw in (dict(model="SABR"), dict(strikes=[]), dict(option_types=["put"]), dict(exercise_every=-2),
               dict(strikes=[100.0, -1.0], option_types="straddle")):
        with pytest.raises(ValueError) as a:
            price_american_chain(**dict(ARGS, **kw))
        with pytest.raises(ValueError) as b:
            price_american_chain_greeks(**dict(ARGS, bump=0.0, **kw))
        assert str(a.value) == str(b.value) and "bump" not in str(b.value)


@pytest.mark.parametrize("kw,match", [(dict(exercise_every=None), "exercise_every"), (dict(exercise_every=[3]), "exercise_every"),
                                      (dict(exercise_every=-1), "exercise_every"), (dict(bump=0.0), "bump"), (dict(K=-1.0), "positive")],
                         ids=["none", "list", "negative", "bump", "strike"])
def test_bermudan_facade_refuses_before_the_device(kw, match):
    from options_model_amd import price_bermudan_greeks
    args = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, exercise_every=2, device=10 ** 6)
    with pytest.raises(ValueError, match=match):
        price_bermudan_greeks(**dict(args, **kw))


def test_facades_are_exported():
    import options_model_amd as oma
    assert callable(oma.price_american_chain_greeks) and callable(oma.price_bermudan_greeks)
    assert {"entries", "strikes", "option_types", "exercise_every", "entry_info", "timings_ms", "info"} == set(
        oma.ChainGreeksResult.__dataclass_fields__)


def test_the_catalogue_calls_the_symbol_of_the_extension_header():
    used = gcat.symbols_used()
    assert set(_ffi.CHAIN_GREEKS_SIGNATURES) == set().union(*used.values()) - {"omc_set_option"}
    for e in gcat.CATALOGUE:
        assert used[e.name] - {"omc_set_option"} == {"omc_" + e.family}, (e.name, used[e.name])
        assert e.name == f"{e.family}/{e.name.split('/')[1]}/{e.cls}"
    assert len({e.name for e in gcat.CATALOGUE}) == len(gcat.CATALOGUE)
    for fam in gcat.FAMILIES:
        assert {e.cls for e in gcat.CATALOGUE if e.family == fam} == {"S", "M"}


# ------------------------------------------------------------------ the view's route against the masked policy's
def test_view_dates():
    assert list(cg.view_dates(13, 5)) == [-2, 3, 8, 13] and list(cg.view_dates(12, 3)) == [0, 3, 6, 9, 12]
    assert list(cg.view_dates(7, 0)) == list(range(8)) == list(cg.view_dates(7, 1))
    assert list(cg.view_dates(7, 7)) == [0, 7] == list(cg.view_dates(7, 10)) and list(cg.view_dates(1, 0)) == [0, 1]
    for N in (1, 2, 7, 12, 13, 70):
        for k in (0, 1, 2, 3, 5, N - 1, N, N + 3):
            assert list(cg.view_dates(N, k)[1:-1]) == list(np.nonzero(br.schedule(N, max(k, 0)))[0]), (N, k)


def _same(a, b, what):
    for key in ("n_exercised", "n_exercised_up", "n_exercised_down", "n_zero", "n_paths"):
        assert a[key] == b[key], (what, key, a[key], b[key])
    for e in range(3):
        assert np.array_equal(a["tex"][e], b["tex"][e]), (what, e)
    for key in ("price", "sum", "sumsq", "price_up", "price_down", "delta", "gamma", "vega", "rho", "theta", "se_delta",
                "se_gamma", "se_vega", "se_rho", "se_theta"):
        assert abs(a[key] - b[key]) <= 1e-12 * max(1.0, abs(b[key])), (what, key, a[key], b[key])


@pytest.mark.parametrize("N", [7, 12, 13])
@pytest.mark.parametrize("folded", [False, True], ids=["full", "folded"])
def test_view_route_equals_the_masked_policy_on_the_full_matrix(N, folded):
    M = 6000
    for is_put, K in ((True, 100.0), (False, 97.0)):
        if folded:
            S = orc.gbm_paths(M // 2, N, S0, R, SIG, T, seed=11 + N, stream=3, antithetic=0)
            c0, g = orc.fold_constants(S0, K, R, SIG, T, N)
            fit = orc.lsm_two_pass_folded(S, K, R, T, is_put, c0, g)
            cK = orc.fold_table(N, c0, g)
        else:
            S = orc.gbm_paths(M, N, S0, R, SIG, T, seed=11 + N, stream=3)
            fit = orc.lsm_poly(S, K, R, T, is_put, "two_pass")
            cK = None
        b4 = gr.betas4_from(fit["betas"], fit["nitm"])
        american = gr.greeks(S, K, R, T, is_put, b4, S0, SIG, h=0.02, cK=cK)
        _same(cg.view_greeks(S, K, R, T, is_put, b4, S0, SIG, h=0.02, every=0, cK=cK), american, (N, "american"))
        seen = set()
        for k in (2, 3, 5, N - 1, N, N + 3):
            mb = cg.masked(b4, k)
            assert np.array_equal(mb[br.schedule(N, k)], b4[br.schedule(N, k)]) and not mb[~br.schedule(N, k)].any()
            ref = gr.greeks(S, K, R, T, is_put, mb, S0, SIG, h=0.02, cK=cK)
            view = cg.view_greeks(S, K, R, T, is_put, b4, S0, SIG, h=0.02, every=k, cK=cK)   # (reads the scheduled rows only)
            _same(view, ref, (N, k, is_put, folded))
            if k >= N:
                assert view["n_exercised"] == view["n_exercised_up"] == view["n_exercised_down"] == 0
            seen.add(view["n_exercised"])
        assert len(seen) > 2 or not is_put   # the schedules differ


def test_heston_entries_have_no_vega_rho_theta():
    S = orc.gbm_paths(2000, 7, S0, R, SIG, T, seed=3)
    fit = orc.lsm_poly(S, 100.0, R, T, True, "two_pass")
    v = cg.view_greeks(S, 100.0, R, T, True, gr.betas4_from(fit["betas"], fit["nitm"]), S0, None, every=3, gbm=False)
    assert all(np.isnan(v[k]) and np.isnan(v["se_" + k]) for k in ("vega", "rho", "theta")) and np.isfinite(v["delta"])


# ------------------------------------------------------------------ the fuzz cases
CASES = cg.fuzz_cases(8, 353535)


def test_fuzz_cases_cover_the_list():
    assert {c["folded"] for c in CASES} == {True, False} and {c["model"] for c in CASES} == {"gbm", "heston"}
    assert {c["scheme"] for c in CASES if c["model"] == "heston"} == {0, 1, 3}
    assert {(c["M"] // 2) % 2 for c in CASES if c["folded"]} == {0, 1}           # both column widths of the folded sweep
    assert min(len(c["strikes"]) for c in CASES) == 1 and max(len(c["strikes"]) for c in CASES) > 16
    assert any(c["r"] == 0.0 for c in CASES) and any(c["pair_offset"] for c in CASES)
    for c in CASES:
        assert c["M"] % 2 == 0 and 1 <= c["N"] <= 70 and 0.001 <= c["bump"] <= 0.5
        assert all(0.7 * c["S0"] <= k <= 1.3 * c["S0"] for k in c["strikes"]) and all(0 <= k <= c["N"] + 3 for k in c["every"])
    assert any(k >= 2 for c in CASES for k in c["every"]) and any(k < 2 for c in CASES for k in c["every"])


@pytest.mark.parametrize("i", range(len(CASES)))
def test_fuzz_cases_are_free_of_ties_on_the_restatement(i):
    """every decision of every entry's three scenarios lies more than 1e-10 K from its continuation value, on the oracle's
    paths with the oracle's fits: the device and the restatement cannot differ by a tie"""
    c = CASES[i]
    S = br.oracle_paths(c, half=c["folded"])
    for K, put, k in zip(c["strikes"], c["puts"], c["every"]):
        if c["folded"]:
            c0, g = orc.fold_constants(c["S0"], K, c["r"], c["sigma"], c["T"], c["N"])
            fit = orc.lsm_two_pass_folded(S, K, c["r"], c["T"], put, c0, g)
            cK = orc.fold_table(c["N"], c0, g)
        else:
            fit = orc.lsm_poly(S, K, c["r"], c["T"], put, "two_pass")
            cK = None
        v = cg.view_greeks(S, K, c["r"], c["T"], put, gr.betas4_from(fit["betas"], fit["nitm"]), c["S0"], c["sigma"], h=c["bump"],
                           every=k, cK=cK, gbm=c["model"] == "gbm")
        assert v["ties"] == [0, 0, 0], (i, K, put, k, v["ties"])

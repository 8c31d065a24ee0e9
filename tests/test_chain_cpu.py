"""CPU suite: the option-chain entry points (omc_price_american_chain, omc_chain_width) are exported
and bound, the ABI number moved with them, the facade refuses bad chains before it touches the library, and the random
chains of tests/test_gpu_chain_fuzz.py cover what that sweep is there for."""
import ctypes as C

import pytest

from helpers import chain_cases as cc
from options_model_amd import _ffi


def test_library_exports_the_chain_entry_points():
    lib = _ffi.load_library()
    for s in ("omc_price_american_chain", "omc_chain_width"):
        assert hasattr(lib, s) and s in _ffi.SIGNATURES


def test_abi_version_is_14():
    assert _ffi.load_library().omc_abi_version() == 14 == _ffi.ABI_VERSION


def test_chain_struct_layouts():
    assert C.sizeof(_ffi.ChainEntry) == 16
    assert C.sizeof(_ffi.ChainInfo) == 48


@pytest.mark.parametrize("kw,match", [
    (dict(strikes=[]), "empty"),
    (dict(strikes=[100.0, 0.0]), "positive"),
    (dict(strikes=[100.0, -5.0]), "positive"),
    (dict(strikes=[100.0, float("nan")]), "positive"),
    (dict(strikes=[100.0], option_types="straddle"), "option_type"),
    (dict(strikes=[90.0, 100.0], option_types=["put", "both"]), "option_type"),
    (dict(strikes=[90.0, 100.0, 110.0], option_types=["put", "call"]), "one per strike"),
    (dict(strikes=[100.0 + i for i in range(257)]), "at most 256"),
])
def test_facade_refuses_bad_chains_without_a_device(monkeypatch, kw, match):
    import options_model_amd
    from options_model_amd import api

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_ffi, "default_context", no_library)
    monkeypatch.setattr(_ffi, "load_library", no_library)
    args = dict(S0=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=10_000, n_steps=50)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        options_model_amd.price_american_chain(**args)
    assert options_model_amd.ChainResult is api.ChainResult


@pytest.mark.parametrize("seed", [171717, 0, 1, 2, 3, 20250101, 2 ** 31 - 1])
@pytest.mark.parametrize("n", [8, 40])
def test_chain_generator_covers_storage_sides_and_duplicates(seed, n):
    cases = cc.chain_cases(n, seed)
    assert len(cases) == n
    head = cases[:8]
    assert sum(cc.is_folded(c) for c in head) >= 3 and sum(not cc.is_folded(c) for c in head) >= 2
    assert any(cc.is_folded(c) and (c["M"] // 2) % 4 == 0 for c in head)     # 16-byte loads
    assert any(cc.is_folded(c) and (c["M"] // 2) % 4 != 0 for c in head)     # scalar loads
    assert {c["M"] for c in head} >= {cc.FOLD_MIN_PATHS}
    assert any(all(c["sides"]) for c in head) and any(len(set(c["sides"])) == 2 for c in head)
    assert any(cc.has_duplicate(c) and cc.is_folded(c) for c in head)
    assert {len(c["strikes"]) for c in head} >= {1, 12}
    assert {c["chain_k"] for c in head} == {-1, 1, 2, 3, 16}
    for c in cases:
        assert c["M"] % 2 == 0 and 2 <= c["M"] <= 300_000 and 2 <= c["N"] <= 80
        assert 1 <= len(c["strikes"]) == len(c["sides"]) <= 12
        assert all(0.5 * c["S0"] <= k <= 1.6 * c["S0"] for k in c["strikes"])


def test_c_chain_example_compiles_against_the_header_and_library(tmp_path):
    import os
    import shutil
    import subprocess

    from options_model_amd import _build
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_chain"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_chain.c"), "-o", str(exe), "-L", os.path.dirname(lib), "-lomc",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    assert exe.exists()

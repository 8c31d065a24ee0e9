"""The case generator of tests/test_gpu_basket_bounds_fuzz.py, checked without a GPU: what the sweep claims to cover."""
import numpy as np

from helpers import basket_bounds_case as bc


def test_default_sweep_covers_what_it_claims():
    cases = bc.fuzz_cases(12)
    assert len(cases) == 12
    assert {c["d"] for c in cases} == set(range(1, 9))
    assert {c["kind"] for c in cases} == set(bc.KINDS)
    assert {c["policy"] for c in cases} == set(bc.POLICIES)
    assert 3 * sum(c["refill"] for c in cases) >= len(cases)  # at least a third refill lanes
    assert all(c["refill"] == (c["n_inner"] // 2 > 64) for c in cases)
    assert {c["n_inner"] for c in cases} <= set(bc.N_INNER) and 2 in {c["n_inner"] for c in cases}
    assert all(1 <= c["N"] <= 13 and c["n_outer"] % 2 == 0 and c["n_lower"] % 2 == 0 and c["M"] % 2 == 0 for c in cases)
    assert any(c["n_outer"] % 8 for c in cases)  # ragged: no multiple of the widest store
    assert any(c["irr_every"] for c in cases) and any(not c["irr_every"] for c in cases)
    assert any(any(c["holes"]) for c in cases if c["policy"] == "given")
    assert {c["is_put"] for c in cases} == {True, False}


def test_cases_are_seeded_and_valid():
    a, b = bc.fuzz_cases(24), bc.fuzz_cases(24)
    assert [{k: v for k, v in c.items() if k != "rho"} for c in a] == [{k: v for k, v in c.items() if k != "rho"} for c in b]
    assert a[:12] != bc.fuzz_cases(12, seed=1)[:12]
    for c in a:
        d = c["d"]
        assert len(c["S0"]) == len(c["sigma"]) == len(c["q"]) == len(c["w"]) == d and c["rho"].shape == (d, d)
        assert np.allclose(np.diag(c["rho"]), 1.0) and np.array_equal(c["rho"], c["rho"].T)
        assert np.linalg.eigvalsh(c["rho"]).min() > 0.05  # the library's Cholesky pivots stay far above 1e-12
        assert all(x > 0 for x in c["S0"] + c["sigma"] + c["w"]) and len(c["holes"]) == c["N"] + 1


def test_prefix_property():
    """a longer sweep starts with the shorter one: OMC_FUZZ_SCALE adds cases, it does not change them"""
    a, b = bc.fuzz_cases(12), bc.fuzz_cases(24)
    assert [c["seed"] for c in a] == [c["seed"] for c in b[:12]]

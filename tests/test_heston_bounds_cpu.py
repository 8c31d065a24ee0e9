"""What omc_price_american_bounds_heston and omc_heston_paths_sv_f32 offer without a GPU: the symbols
and the ABI version, the facade's argument checks, the pair and row indexing of the test helper that rebuilds the inner
paths (tests/helpers/heston_bounds_case.py) on fake normals and a fake spot builder, and the fuzz cases."""
import numpy as np
import pytest

from helpers import heston_bounds_case as hc
from options_model_amd import _ffi

K = 100.0


# ------------------------------------------------------------------ the interface
def test_symbols_and_abi_version():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(lib.omc_price_american_bounds_heston.argtypes) == 8
    assert len(lib.omc_heston_paths_sv_f32.argtypes) == 18
    assert len(lib.omc_heston_paths_sv_f32.argtypes) == len(lib.omc_heston_paths_f32.argtypes) + 1


@pytest.mark.parametrize("kw,match", [
    (dict(n_inner=255), "n_inner"), (dict(n_outer=1023), "n_outer"), (dict(n_lower=99_999), "n_lower"),
    (dict(policy="given"), "betas"), (dict(betas=np.zeros((5, 4))), "betas"), (dict(policy="lattice"), "policy"),
    (dict(heston_scheme="calibrator"), "calibrator"), (dict(heston_scheme="milstein"), "heston_scheme"),
    (dict(policy="given", betas=np.zeros((5, 3))), "shape"), (dict(policy="given", betas=np.zeros((6, 4))), "shape"),
    (dict(option_type="straddle"), "option_type")],
    ids=["odd-inner", "odd-outer", "odd-lower", "given-no-betas", "betas-not-given", "policy", "calibrator", "scheme",
         "betas-cols", "betas-rows", "option-type"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_american_bounds_heston

    args = dict(S0=100.0, K=K, r=0.05, T=1.0, n_paths=1000, n_steps=4, heston_params=hc.HP, device=10 ** 6)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_american_bounds_heston(**args)


def test_context_method_checks_the_betas_shape():
    ctx = object.__new__(_ffi.Context)  # never opened: the check needs no device
    ctx.handle = None
    with pytest.raises(ValueError, match=r"\(6, 4\)"):
        ctx.price_american_bounds_heston(hc.make_params(hc.HP, N=5), policy="given", betas=np.zeros((5, 4)))


# ------------------------------------------------------------------ the helper's indexing
def test_inner_items_take_their_pairs_rows_and_length():
    """Fake normals that encode (generator pair, row) and a fake spot builder that records what it was given: item (i, t)
    asks for pairs (i (N+1) + t) H .. + H - 1, Heston step k gets rows 2(k-1) and 2(k-1)+1, the start is the outer state,
    and N - t + 1 rows come back."""
    N, n_outer, n_inner = 5, 4, 6
    H = n_inner // 2
    So = (100.0 + np.arange((N + 1) * n_outer, dtype=np.float32)).reshape(N + 1, n_outer)
    Vo = (0.01 * np.arange((N + 1) * n_outer, dtype=np.float32) - 0.05).reshape(N + 1, n_outer)  # some negative
    asked, built = [], []

    def normals(off, n):
        asked.append((off, n))
        rows = np.arange(2 * N, dtype=np.float64)[:, None]
        return (1000.0 * (off + np.arange(n))[None, :] + rows).astype(np.float32)  # value = 1000 pair + row

    def spots(z1, z2, s0, v0):
        built.append((z1.copy(), z2.copy(), s0, v0))
        out = np.zeros((N + 1, 2 * H), np.float32)
        out[:, :] = np.arange(N + 1, dtype=np.float32)[:, None]  # row k holds k
        return out

    inner = hc.inner_from_state(normals, spots, So, Vo, n_inner)
    for i, t in ((0, 0), (1, 2), (3, 4), (2, N - 1)):
        S = inner(i, t)
        off, n = asked[-1]
        assert (off, n) == ((i * (N + 1) + t) * H, H)
        z1, z2, s0, v0 = built[-1]
        assert z1.shape == z2.shape == (N, H) and z1.flags["C_CONTIGUOUS"] and z2.flags["C_CONTIGUOUS"]
        for k in range(1, N + 1):
            np.testing.assert_array_equal(z1[k - 1], 1000.0 * (off + np.arange(H)) + 2 * (k - 1))
            np.testing.assert_array_equal(z2[k - 1], 1000.0 * (off + np.arange(H)) + 2 * (k - 1) + 1)
        assert s0 == float(So[t, i]) and v0 == float(Vo[t, i])
        assert np.float32(v0) == Vo[t, i]  # a float32 is exact in the double argument
        assert S.shape == (N - t + 1, n_inner)
        np.testing.assert_array_equal(S[:, 0], np.arange(N - t + 1))  # rows 0 .. N - t, in order
    assert Vo.min() < 0  # the negative scheme-1 state passes through unchanged


def test_inner_matches_bounds_ref_item_layout():
    """the pair offset of an item is bounds_ref.inner_by_item's: the two helpers address the same generator pairs"""
    from helpers import bounds_ref as br

    N, n_inner = 3, 4
    So = np.full((N + 1, 6), 100.0, np.float32)
    a, b = [], []
    br.inner_by_item(lambda off, n: a.append((off, n)) or np.zeros((N, n), np.float32), So, n_inner,
                     lambda z, s0: np.zeros((N + 1, n_inner), np.float32))(4, 2)
    hc.inner_from_state(lambda off, n: b.append((off, n)) or np.zeros((2 * N, n), np.float32),
                        lambda z1, z2, s0, v0: np.zeros((N + 1, n_inner), np.float32), So, So, n_inner)(4, 2)
    assert a == b == [((4 * (N + 1) + 2) * 2, 2)]


# ------------------------------------------------------------------ the fuzz cases
def test_fuzz_cases_cover_what_they_promise():
    cases = hc.fuzz_cases(8)
    assert cases == hc.fuzz_cases(8)  # seeded: the same cases every time
    assert cases == hc.fuzz_cases(12)[:8]
    assert all(1 <= c["N"] <= 13 and c["n_inner"] in hc.N_INNER for c in cases)
    assert all(c["n_outer"] % 2 == 0 and 2 <= c["n_outer"] <= 40 and c["n_lower"] % 2 == 0 and c["M"] % 2 == 0 for c in cases)
    assert {c["n_inner"] for c in cases} == set(hc.N_INNER) and len({c["n_outer"] for c in cases}) > 3
    assert 3 * sum(c["refill"] for c in cases) >= len(cases)
    assert {c["scheme"] for c in cases} == {0, 1} and {c["is_put"] for c in cases} == {True, False}
    assert {c["policy"] for c in cases} == set(hc.POLICIES)
    given = [c for c in cases if c["policy"] == "given"]
    assert len(given) == len(cases) // 4 and all(len(c["holes"]) == c["N"] + 1 for c in cases)
    assert any(any(c["holes"][1:c["N"]]) for c in given)
    assert any(c["irr_every"] for c in cases) and not all(c["irr_every"] for c in cases)
    for k, c in enumerate(cases):
        assert c["feller"] == (k % 3 != 2) and c["feller"] == (2 * c["kappa"] * c["theta"] >= c["xi"] ** 2)
        assert 0.8 <= c["S0"] / c["K"] <= 1.25 and -1.0 <= c["rho"] <= 1.0 and c["v0"] >= 0
        p = hc.fuzz_params(c)
        assert p.model == _ffi.MODELS["heston"] and p.heston_scheme == c["scheme"] and p.antithetic == 1
        assert (p.n_steps, p.n_paths, p.xi) == (c["N"], c["M"], c["xi"])

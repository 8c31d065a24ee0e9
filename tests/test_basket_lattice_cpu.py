"""The lattices of tests/helpers/basket_lattice.py, which the multi-asset bound tests bracket (test_gpu_basket_bounds.py):
the Boyle-Evnine-Gibbs two-asset lattice against the published values of the max-call benchmark (Broadie-Glasserman /
Andersen-Broadie 2004: two assets, S0 = 90 / 100 / 110, K = 100, r = 5 %, yield 10 %, sigma = 20 %, rho = 0, T = 3, nine
exercise dates: 8.075 / 13.902 / 21.345), against the one-asset lattice of bounds_ref where the second asset cannot matter,
and the orderings of best-of and worst-of against the single assets."""
import pytest

from helpers import basket_lattice as bl
from helpers import bounds_ref as br

PUBLISHED = {90.0: 8.075, 100.0: 13.902, 110.0: 21.345}
BENCH = dict(K=100.0, r=0.05, sigmas=(0.2, 0.2), T=3.0, n_dates=9, yields=(0.1, 0.1), rho=0.0, kind="best-of", is_put=False)


@pytest.fixture(scope="module")
def benchmark():
    """{m: {S0: value}} at 40 and 80 lattice steps per exercise date, computed once."""
    return {m: {s: bl.two_asset((s, s), m=m, **BENCH) for s in PUBLISHED} for m in (40, 80)}


def test_two_resolutions_agree(benchmark):
    for s in PUBLISHED:
        assert abs(benchmark[40][s] - benchmark[80][s]) <= 0.01, (s, benchmark)


def test_published_max_call_values(benchmark):
    for s, v in PUBLISHED.items():
        assert abs(benchmark[80][s] - v) <= 0.01, (s, benchmark[80][s], v)


def test_negligible_second_asset_is_the_one_asset_lattice():
    """Best-of put with a second asset of weight 1e-9 (w_2 S_2 never reaches w_1 S_1, so the index is asset 1) against the
    Gaussian-weight lattice of bounds_ref (q = 0), whose own error is far below a binomial lattice's, to the two-asset
    lattice's own resolution difference |V(2 m) - V(m)|.  m = 80 is the resolution the bracket tests of
    tests/test_gpu_basket_bounds.py take their reference values at, and 2 m = 160 is its doubling: the pair that says how
    far that reference can be trusted.  (Measured: |V(160) - ref| = 0.001621 against |V(160) - V(80)| = 0.001622; an error
    that falls like 1 / m makes the two equal to leading order.)"""
    args = dict(S0=(100.0, 100.0), K=100.0, r=0.05, sigmas=(0.2, 0.3), T=1.0, n_dates=4, weights=(1.0, 1e-9),
                kind="best-of", is_put=True)
    coarse, fine = bl.two_asset(m=80, **args), bl.two_asset(m=160, **args)
    ref = br.lattice(100.0, 100.0, 0.05, 0.2, 1.0, 4, is_put=True)
    print(coarse, fine, ref)
    assert abs(fine - ref) <= abs(fine - coarse), (coarse, fine, ref)


def test_one_asset_lattice_without_yield_is_bounds_ref():
    """the one-asset lattice with q = 0 against bounds_ref.lattice, to its own resolution difference |V(200) - V(100)|"""
    args = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_dates=4, is_put=True)
    coarse, fine = bl.one_asset(m=100, **args), bl.one_asset(m=200, **args)
    ref = br.lattice(100.0, 100.0, 0.05, 0.2, 1.0, 4, is_put=True)
    print(coarse, fine, ref)
    assert abs(fine - ref) <= abs(fine - coarse), (coarse, fine, ref)


@pytest.mark.parametrize("rho", [-0.3, 0.0, 0.5])
def test_best_of_and_worst_of_against_the_single_assets(rho):
    """A call pays more on the larger index: best-of call >= either asset's own call >= worst-of call (the same game on
    each: dates, rate, yields).  The two assets differ, so every inequality holds by dollars, not by lattice error."""
    common = dict(K=100.0, r=0.05, T=1.0, n_dates=4)
    S0, sig, q = (100.0, 95.0), (0.2, 0.3), (0.04, 0.08)
    single = [bl.one_asset(S0[k], sigma=sig[k], q=q[k], m=40, is_put=False, **common) for k in range(2)]
    best = bl.two_asset(S0, sigmas=sig, yields=q, rho=rho, kind="best-of", m=20, is_put=False, **common)
    worst = bl.two_asset(S0, sigmas=sig, yields=q, rho=rho, kind="worst-of", m=20, is_put=False, **common)
    print(rho, single, best, worst)
    assert best >= max(single) and worst <= min(single)
    basket = bl.two_asset(S0, sigmas=sig, yields=q, rho=rho, kind="basket", weights=(0.5, 0.5), m=20, is_put=False, **common)
    assert worst <= basket <= best

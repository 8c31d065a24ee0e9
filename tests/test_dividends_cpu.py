"""Dividends without a GPU (include/omc.h "dividends"): the new symbols and struct layouts, the
host-side schedule of omc_dividend_schedule against its restatement (tests/helpers/dividend_ref.py) bit for bit, every
refusal code, the restatement itself against Black-Scholes-Merton on C-oracle paths, the case generator of the device
sweep (tests/test_gpu_dividends_fuzz.py) and the C example."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_dividends_fuzz as fz
from helpers import dividend_ref as dr
from oracle import cpu as orc
from options_model_amd import _build, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(T=1.0, N=12, **kw):
    kw.setdefault("semantics", "two_pass")
    return _ffi.make_params(n_paths=1000, n_steps=N, T=T, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_table(T, N, divs, q=0.0):
    mul, cash, has = _ffi.dividend_schedule(_params(T, N), q, divs)
    rm, rc, rh = dr.schedule(T, N, divs)
    assert np.array_equal(_bits(mul), _bits(rm)), (T, N, divs)
    assert np.array_equal(_bits(cash), _bits(rc)), (T, N, divs)
    assert np.array_equal(has, rh), (T, N, divs)
    return mul, cash, has


# ------------------------------------------------------------------ ABI
def test_symbols_structs_and_version():
    lib = _ffi.load_library()
    for s in ("omc_dividend_schedule", "omc_price_american_div"):
        assert hasattr(lib, s) and s in _ffi.SIGNATURES
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert C.sizeof(_ffi.Dividend) == 24
    assert C.sizeof(_ffi.DivResult) == C.sizeof(_ffi.Result) + 16
    assert _ffi.DivResult.base.offset == 0 and _ffi.DivResult.ms_div_paths.offset == C.sizeof(_ffi.Result)
    assert issubclass(_ffi.DividendError, _ffi.OmcError) and issubclass(_ffi.DividendError, ValueError)
    import options_model_amd
    assert callable(options_model_amd.price_american_dividends) and options_model_amd.DividendResult is not None


# ------------------------------------------------------------------ the schedule
def test_schedule_edges():
    T, N = 1.0, 12
    # t = T and t just above 0: the last and the first step
    _, _, has = _same_table(T, N, [(T, 1.0), (5e-324, 0.1, "proportional")])
    assert list(np.nonzero(has)[0]) == [1, N]
    _, _, has = _same_table(T, N, [(1e-12, 2.0)])
    assert list(np.nonzero(has)[0]) == [1]
    # exactly on a grid time, and one ulp either side of it: the same step (the 1e-9 slack of the rule)
    for k in (1, 3, 7, N):
        g = k * T / N
        for t in (g, np.nextafter(g, 0.0), np.nextafter(g, 2.0) if k < N else g):
            _, _, has = _same_table(T, N, [(float(t), 1.5)])
            assert list(np.nonzero(has)[0]) == [k], (k, t)
    # strictly inside an interval: the step that ends it
    _, _, has = _same_table(T, N, [(0.26, 1.0)])
    assert list(np.nonzero(has)[0]) == [4]
    # no dividends at all: the identity table
    mul, cash, has = _same_table(T, N, [], q=0.03)
    assert np.all(mul == 1.0) and np.all(cash == 0.0) and not has.any()
    # a zero-amount dividend: an entry (has) whose factors are the identity
    mul, cash, has = _same_table(T, N, [(0.25, 0.0), (0.5, 0.0, "proportional")])
    assert has.sum() == 2 and np.all(mul == 1.0) and np.all(cash == 0.0)


def test_three_dividends_on_one_step_compose_in_input_order():
    T, N = 2.0, 8
    a = [(0.5, 1.0, "cash"), (0.45, 0.1, "proportional"), (0.5, 2.0, "cash")]
    mul, cash, has = _same_table(T, N, a)
    assert list(np.nonzero(has)[0]) == [2]
    assert mul[2] == np.float32(0.9) and cash[2] == np.float32(1.0 * 0.9 + 2.0)
    mul, cash, has = _same_table(T, N, a[::-1])
    assert mul[2] == np.float32(0.9) and cash[2] == np.float32(2.0 * 0.9 + 1.0)
    # unsorted input over several steps: sorted by step, input order kept within one
    b = [(1.9, 0.5), (0.1, 0.02, "proportional"), (1.0, 0.3), (0.1, 0.7), (1.0, 0.05, "proportional"), (0.3, 0.01, "proportional")]
    mul, cash, has = _same_table(T, N, b)
    assert list(np.nonzero(has)[0]) == [1, 2, 4, 8]
    assert cash[1] == np.float32(0.7) and mul[1] == np.float32(0.98) and cash[4] == np.float32(0.3 * 0.95)


def test_schedule_random_sweep():
    rng = np.random.default_rng(20260314)
    for _ in range(200):
        T = float(rng.choice([0.1, 0.5, 1.0, 1.0 / 3.0, 2.5, 7.0]))
        N = int(rng.choice([1, 2, 3, 7, 12, 50, 64, 252, 1000]))
        divs = []
        for _ in range(int(rng.integers(0, 9))):
            t = float(rng.choice([rng.uniform(1e-9, T), T, rng.integers(1, N + 1) * T / N]))
            t = min(max(t, 1e-300), T)
            if rng.random() < 0.5:
                divs.append((t, float(rng.uniform(0.0, 5.0)), "cash"))
            else:
                divs.append((t, float(rng.uniform(0.0, 0.3)), "proportional"))
        _same_table(T, N, divs, q=float(rng.uniform(-0.05, 0.1)))


# ------------------------------------------------------------------ refusals
def _rc(p, q, d, n):
    lib = _ffi.load_library()
    return lib.omc_dividend_schedule(C.byref(p) if p is not None else None, q, d, n, None, None, None)


def test_every_invalid_input_returns_its_code():
    ok = _params()
    one = lambda t, a, k: (_ffi.Dividend * 1)(_ffi.Dividend(t, a, k, 0))  # noqa: E731
    assert _rc(ok, 0.02, one(0.5, 1.0, 1), 1) == 0 and _rc(ok, -0.02, None, 0) == 0
    assert _rc(None, 0.0, None, 0) == -7
    for q in (math.nan, math.inf, -math.inf):
        assert _rc(ok, q, None, 0) == -17
    assert _rc(ok, 0.0, None, -1) == -18
    assert _rc(ok, 0.0, None, 2) == -19
    for t in (0.0, -0.5, 1.0000001, math.nan, math.inf):
        assert _rc(ok, 0.0, one(t, 1.0, 1), 1) == -20, t
    for a in (-1e-9, math.nan, math.inf):
        assert _rc(ok, 0.0, one(0.5, a, 1), 1) == -21, a
        assert _rc(ok, 0.0, one(0.5, a, 0), 1) == -21, a
    for a in (1.0, 1.5):
        assert _rc(ok, 0.0, one(0.5, a, 0), 1) == -22, a
    assert _rc(ok, 0.0, one(0.5, 1.5, 1), 1) == 0  # a cash amount has no such bound
    for k in (-1, 2, 77):
        assert _rc(ok, 0.0, one(0.5, 0.1, k), 1) == -23, k
    assert _rc(_params(antithetic=False), 0.0, None, 0) == -24
    for sem in ("reference", "textbook"):
        assert _rc(_params(semantics=sem), 0.0, None, 0) == -11
    # the omc_params checks of omc_price_american
    assert _rc(_params(S0=-1.0), 0.0, None, 0) == -1 and _rc(_params(r=-0.01), 0.0, None, 0) == -2
    assert _rc(_params(N=0), 0.0, None, 0) == -3 and _rc(_params(N=5000), 0.0, None, 0) == -8
    assert _rc(_params(sigma=0.0), 0.0, None, 0) == -5
    # the Python binding raises for them: an OmcError that is also a ValueError, with the code
    with pytest.raises(_ffi.OmcError) as e:
        _ffi.dividend_schedule(ok, 0.0, [(0.5, 1.0, "proportional")])
    assert e.value.code == -22 and isinstance(e.value, ValueError)
    with pytest.raises(_ffi.OmcError):
        _ffi.dividend_schedule(ok, 0.0, [(0.5, 1.0, "scrip")])
    with pytest.raises(ValueError):
        _ffi.dividend_schedule(ok, 0.0, [(0.5,)])


# ------------------------------------------------------------------ the restatement itself
@pytest.fixture(scope="module")
def oracle_paths():
    q = 0.03
    M, N = 200_000, 8
    return {qq: orc.gbm_paths(M, N, 100.0, 0.05 - qq, 0.2, 1.0, 77, 2) for qq in (0.0, q)}


@pytest.mark.parametrize("q,divs", [(0.03, []), (0.0, [(0.3, 0.02, "proportional"), (0.8, 0.035, "proportional")]),
                                    (0.03, [(0.3, 0.02, "proportional"), (0.8, 0.035, "proportional")])],
                         ids=["yield", "proportional", "both"])
def test_restatement_prices_the_european_closed_form(oracle_paths, q, divs):
    S0, K, r, sig, T = 100.0, 100.0, 0.05, 0.2, 1.0
    V = oracle_paths[q]
    M, N = V.shape[1], V.shape[0] - 1
    S = dr.apply(V, *dr.schedule(T, N, divs))
    spot = S0 * math.prod(1.0 - d[1] for d in divs)
    for is_put in (True, False):
        s, s2 = orc.european_from_paths(S.astype(np.float32), K, r, T, is_put)
        mean = s / M
        se = math.sqrt(max(s2 / M - mean * mean, 0.0) / M)
        ref = dr.bsm(spot, K, r, q, sig, T, is_put)
        print(f"q={q} divs={len(divs)} put={is_put}: mc {mean:.5f} +- {se:.5f}  bsm {ref:.5f}")
        assert abs(mean - ref) <= 4.0 * se


def test_apply_with_a_zero_dividend_returns_the_vanilla_matrix(oracle_paths):
    V = oracle_paths[0.0][:, :4096]
    N = V.shape[0] - 1
    for divs in ([], [(0.4, 0.0)], [(0.4, 0.0, "proportional"), (1.0, 0.0)]):
        S = dr.apply(V, *dr.schedule(1.0, N, divs))
        assert np.array_equal(S.astype(np.float32), V)  # (the float64 products round back to the float32 spots)
    # and a cash dividend larger than the spot leaves exactly 0 from its step on
    S = dr.apply(V, *dr.schedule(1.0, N, [(0.5, 1e6)]))
    assert np.all(S[4:] == 0.0) and np.array_equal(S[:4].astype(np.float32), V[:4])


def test_bsm_limits():
    assert dr.bsm(100, 100, 0.05, 0.0, 0.2, 1.0, False) == pytest.approx(10.450583572185565, rel=1e-12)
    c, p = dr.bsm(100, 95, 0.03, 0.02, 0.3, 2.0, False), dr.bsm(100, 95, 0.03, 0.02, 0.3, 2.0, True)
    assert c - p == pytest.approx(100 * math.exp(-0.04) - 95 * math.exp(-0.06), rel=1e-12)  # put-call parity


# ------------------------------------------------------------------ the device sweep's case generator
@pytest.mark.parametrize("seed", [fz.SEED, 0, 1, 2, 3, 2 ** 31 - 1])
def test_fuzz_generator_deals_every_code_path(seed):
    cases = fz.cases(fz.N_CASES, seed)
    assert len(cases) == fz.N_CASES
    assert {fz.vec_of(c) for c in cases} == {1, 2, 4}
    assert {(c["model"], c["scheme"]) for c in cases} >= {("gbm", 0), ("heston", 0), ("heston", 1), ("heston", 2)}
    assert {len(c["divs"]) for c in cases} >= {0, 1, 6}
    kinds = {d[2] for c in cases for d in c["divs"]}
    assert kinds == {"cash", "proportional"}
    assert any(c["N"] == 1 for c in cases) and any(c["M"] == 2 for c in cases) and any(c["N"] == 64 for c in cases)
    assert any(c["q"] < 0 for c in cases) and any(c["q"] > 0 for c in cases)
    for c in cases:
        assert 2 <= c["M"] <= 30_000 and c["M"] % 2 == 0 and 1 <= c["N"] <= 64 and len(c["divs"]) <= 6
        p = fz.params(c)
        mul, cash, has = _ffi.dividend_schedule(p, c["q"], c["divs"])  # every case is one the library accepts
        rm, rc, rh = dr.schedule(c["T"], c["N"], c["divs"])
        assert np.array_equal(_bits(mul), _bits(rm)) and np.array_equal(_bits(cash), _bits(rc)) and np.array_equal(has, rh)


# ------------------------------------------------------------------ the C example
def test_c_example_compiles_and_links(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    exe = tmp_path / "american_dividends"
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "american_dividends.c"), "-o", str(exe), "-L", os.path.dirname(lib), "-lomc",
           "-lm", "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.run(cmd, check=True)
    assert exe.exists()

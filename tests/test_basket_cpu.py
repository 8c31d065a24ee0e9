"""Multi-asset options without a GPU (include/omc.h "multi-asset options"): the new symbols and
struct layouts, the host constants of omc_basket_table against their restatement (tests/helpers/basket_ref.py) and
numpy's Cholesky factor, every refusal code, the ValueErrors of price_american_basket, the restatement against the C
oracle's GBM paths, and the C example."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import basket_ref as br
from oracle import cpu as orc
from options_model_amd import _build, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("basket", "geometric", "best-of", "worst-of")


def _params(T=1.0, N=16, M=1000, **kw):
    kw.setdefault("semantics", "two_pass")
    return _ffi.make_params(n_paths=M, n_steps=N, T=T, **kw)


def _equi(d, c):
    return np.full((d, d), c) + (1.0 - c) * np.eye(d)


CASES = [  # (S0, sigma, q, w, rho)
    ([100.0], [0.2], [0.02], [1.0], np.eye(1)),
    ([100.0, 95.0], [0.2, 0.3], [0.0, 0.01], [0.5, 0.5], np.array([[1.0, 0.6], [0.6, 1.0]])),
    ([100.0, 90.0, 110.0], [0.2, 0.25, 0.3], [0.01, 0.0, 0.03], [0.5, 0.3, 0.2],
     np.array([[1.0, 0.5, 0.2], [0.5, 1.0, -0.3], [0.2, -0.3, 1.0]])),
    ([80.0 + 5.0 * i for i in range(8)], [0.15 + 0.02 * i for i in range(8)], [0.005 * i for i in range(8)],
     [0.05 + 0.02 * i for i in range(8)], _equi(8, 0.3)),
]


# ------------------------------------------------------------------ ABI
def test_symbols_structs_and_version():
    lib = _ffi.load_library()
    for s in ("omc_basket_table", "omc_price_american_basket"):
        assert hasattr(lib, s) and s in _ffi.SIGNATURES
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert C.sizeof(_ffi.Basket) == 8 + 8 * (4 * 8 + 64)
    assert C.sizeof(_ffi.BasketResult) == C.sizeof(_ffi.Result) + 24
    assert _ffi.BasketResult.base.offset == 0 and _ffi.BasketResult.ms_basket_paths.offset == C.sizeof(_ffi.Result)
    import options_model_amd
    assert callable(options_model_amd.price_american_basket) and options_model_amd.BasketResult is not None


def test_struct_layouts_match_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "omc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(omc_basket), offsetof(omc_basket, n_assets),\n'
                   '         offsetof(omc_basket, kind), offsetof(omc_basket, S0), offsetof(omc_basket, sigma),\n'
                   '         offsetof(omc_basket, q), offsetof(omc_basket, w), offsetof(omc_basket, rho));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(omc_basket_result), offsetof(omc_basket_result, ms_basket_paths),\n'
                   '         offsetof(omc_basket_result, index0), offsetof(omc_basket_result, n_assets),\n'
                   '         offsetof(omc_basket_result, kind));\n'
                   '  printf("%d %d %d %d\\n", OMC_BASKET_ARITHMETIC, OMC_BASKET_GEOMETRIC, OMC_BASKET_BEST_OF, OMC_BASKET_WORST_OF);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    B, R = _ffi.Basket, _ffi.BasketResult
    assert got == [C.sizeof(B), B.n_assets.offset, B.kind.offset, B.S0.offset, B.sigma.offset, B.q.offset, B.w.offset,
                   B.rho.offset, C.sizeof(R), R.ms_basket_paths.offset, R.index0.offset, R.n_assets.offset, R.kind.offset,
                   0, 1, 2, 3]
    assert [_ffi.BASKET_KINDS[k] for k in KINDS] == [0, 1, 2, 3]


# ------------------------------------------------------------------ the host constants
@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("kind", KINDS)
def test_table_matches_the_restatement(case, kind):
    S0, sig, q, w, rho = CASES[case]
    r, T, N = 0.05, 1.5, 37
    L, a, b, x0, geo = _ffi.basket_table(_params(T, N, r=r), _ffi.make_basket(S0, sig, q, w, rho, kind))
    rL, ra, rb, rx0, rgeo = br.table(S0, sig, q, w, rho, kind, r, T, N)
    assert np.abs(L - np.linalg.cholesky(rho)).max() <= 1e-14 and np.abs(L - rL).max() <= 1e-14
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L)) and L[0, 0] == 1.0
    assert a.dtype == b.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), ra.view(np.uint32)) and np.array_equal(b.view(np.uint32), rb.view(np.uint32))
    assert x0 == pytest.approx(rx0, rel=1e-15)
    for got, want in zip(geo, rgeo):
        assert got == pytest.approx(want, rel=1e-15)
    # the constants are the vanilla generator's at rate r - q_i (oracle/omc_oracle.c: orc_gbm_paths_f32)
    dt = T / N
    for i in range(len(S0)):
        assert a[i] == np.float32(((r - q[i]) - 0.5 * sig[i] ** 2) * dt * br.L2E) and b[i] == np.float32(sig[i] * math.sqrt(dt) * br.L2E)
    # independent statements of the geometric basket's GBM and of the index
    ws, wv, sv = np.array(w) * np.array(S0), np.array(w), np.array(sig)
    assert geo[0] == pytest.approx(math.exp(float(np.sum(wv * np.log(S0)))), rel=1e-13)
    assert geo[1] ** 2 == pytest.approx(float((wv * sv) @ np.asarray(rho) @ (wv * sv)), rel=1e-13)
    assert geo[2] == pytest.approx(r - float(np.sum(wv * (r - np.array(q) - sv ** 2 / 2))) - geo[1] ** 2 / 2, abs=1e-15)
    assert x0 == pytest.approx(dict(zip(KINDS, (ws.sum(), geo[0], ws.max(), ws.min())))[kind], rel=1e-14)


def test_listed_cholesky_factor():
    L = _ffi.basket_table(_params(), _ffi.make_basket([100.0, 100.0], [0.2, 0.2], correlation=[[1.0, 0.6], [0.6, 1.0]]))[0]
    assert L[0, 0] == 1.0 and L[0, 1] == 0.0 and L[1, 0] == 0.6 and L[1, 1] == pytest.approx(0.8, rel=1e-15)
    # a single asset with weight 1 is its own index, and its geometric GBM is the asset's
    _, _, _, x0, geo = _ffi.basket_table(_params(r=0.05), _ffi.make_basket([123.0], [0.25], [0.02], [1.0], kind="geometric"))
    assert x0 == 123.0 and geo[0] == 123.0 and geo[1] == 0.25 and geo[2] == pytest.approx(0.02, abs=1e-15)


def test_table_outputs_may_be_null():
    lib = _ffi.load_library()
    p, b = _params(), _ffi.make_basket([100.0, 90.0], [0.2, 0.3], kind="best-of")
    assert lib.omc_basket_table(C.byref(p), C.byref(b), None, None, None, None, None) == 0
    x0 = C.c_double()
    assert lib.omc_basket_table(C.byref(p), C.byref(b), None, None, None, C.byref(x0), None) == 0 and x0.value == 100.0


# ------------------------------------------------------------------ refusals
def _rc(p, b):
    lib = _ffi.load_library()
    return lib.omc_basket_table(C.byref(p) if p is not None else None, C.byref(b) if b is not None else None, None, None, None,
                                None, None)


def _basket(d=2, **kw):
    args = dict(spots=[100.0] * d, sigmas=[0.2] * d, yields=[0.01] * d, weights=[1.0 / d] * d, correlation=_equi(d, 0.3))
    args.update(kw)
    return _ffi.make_basket(**args)


def test_every_invalid_input_returns_its_code():
    ok = _params()
    assert _rc(ok, _basket()) == 0 and _rc(ok, _basket(8)) == 0 and _rc(ok, _basket(1)) == 0
    assert _rc(ok, _basket(yields=[-0.02, 0.5])) == 0  # a yield of any sign
    assert _rc(None, _basket()) == -7
    assert _rc(ok, None) == -29
    for d in (0, -1, 9):
        b = _basket()
        b.n_assets = d
        assert _rc(ok, b) == -29, d
    for field, bad in (("spots", (0.0, -1.0, math.nan, math.inf)), ("sigmas", (0.0, -0.1, math.nan, math.inf)),
                       ("yields", (math.nan, math.inf, -math.inf)), ("weights", (0.0, -0.5, math.nan, math.inf))):
        for x in bad:
            for at in (0, 1):
                v = [0.3, 0.3]
                v[at] = x
                assert _rc(ok, _basket(**{field: v})) == -30, (field, x, at)
    for kind in (-1, 4, 17):
        assert _rc(ok, _basket(kind=kind)) == -32
    for k in range(4):
        assert _rc(ok, _basket(kind=k)) == 0
    # rho: not finite, diagonal off 1, asymmetric, not positive definite
    assert _rc(ok, _basket(correlation=[[1.0, math.nan], [math.nan, 1.0]])) == -31
    assert _rc(ok, _basket(correlation=[[1.0, math.inf], [math.inf, 1.0]])) == -31
    assert _rc(ok, _basket(correlation=[[1.0 + 1e-9, 0.3], [0.3, 1.0]])) == -31
    assert _rc(ok, _basket(correlation=[[1.0, 0.3], [0.3, 0.999]])) == -31
    assert _rc(ok, _basket(correlation=[[1.0 + 1e-13, 0.3], [0.3, 1.0]])) == 0
    assert _rc(ok, _basket(correlation=[[1.0, 0.3], [0.3 + 1e-9, 1.0]])) == -31
    assert _rc(ok, _basket(correlation=[[1.0, 0.3], [0.3 + 1e-13, 1.0]])) == 0
    assert _rc(ok, _basket(correlation=[[1.0, 1.0], [1.0, 1.0]])) == -31  # singular: the second pivot is 0
    assert _rc(ok, _basket(correlation=[[1.0, -1.2], [-1.2, 1.0]])) == -31
    npd = [[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]]
    assert _rc(ok, _basket(3, correlation=npd)) == -31
    with pytest.raises(ValueError):
        br.cholesky(npd)
    # omc_params: model, the ordinary checks (on the copy: S0 and sigma of the params are not read), flow, layout
    assert _rc(_params(model="heston"), _basket()) == -12
    assert _rc(_params(S0=-1.0, sigma=0.0), _basket()) == 0
    assert _rc(_params(K=-1.0), _basket()) == -1 and _rc(_params(r=-0.01), _basket()) == -2
    assert _rc(_params(N=0), _basket()) == -3 and _rc(_params(N=5000), _basket()) == -8
    assert _rc(_params(M=1001), _basket()) == -3
    assert _rc(_params(antithetic=False), _basket()) == -24
    for sem in ("reference", "textbook"):
        assert _rc(_params(semantics=sem), _basket()) == -11
    # the pair range: pair_offset + n_paths / 2 may reach 2^40 and not pass it
    lim = 1 << 40
    assert _rc(_params(M=1000, pair_offset=lim - 500), _basket()) == 0
    assert _rc(_params(M=1000, pair_offset=lim - 499), _basket()) == -33
    assert _rc(_params(M=1000, pair_offset=lim + 5), _basket()) == -33
    assert _rc(_params(M=1000, pair_offset=(1 << 64) - 1), _basket()) == -33
    # the pricing call refuses a null context and a null result before anything else
    lib = _ffi.load_library()
    out = _ffi.BasketResult()
    assert lib.omc_price_american_basket(None, C.byref(ok), C.byref(_basket()), C.byref(out), None, None, 0) == -7
    # the Python binding raises ValueError for every one of them
    for bad in (_basket(spots=[100.0, -1.0]), _basket(kind=7), _basket(3, correlation=npd)):
        with pytest.raises(ValueError):
            _ffi.basket_table(ok, bad)
    for kw in (dict(spots=[1.0] * 9, sigmas=[0.2] * 9), dict(spots=[], sigmas=[]), dict(spots=[1.0, 2.0], sigmas=[0.2]),
               dict(spots=[1.0, 2.0], sigmas=[0.2, 0.2], correlation=np.eye(3)),
               dict(spots=[1.0, 2.0], sigmas=[0.2, 0.2], weights=[1.0])):
        with pytest.raises(ValueError):
            _ffi.make_basket(**kw)


def test_facade_refuses_bad_arguments_before_any_device_work(monkeypatch):
    from options_model_amd import price_american_basket

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    base = dict(spots=[100.0, 95.0], K=100.0, r=0.05, sigmas=[0.2, 0.3], T=1.0, n_paths=4096, n_steps=20)
    npd = [[1.0, 0.9, 0.9], [0.9, 1.0, -0.9], [0.9, -0.9, 1.0]]
    for kw in (dict(kind="rainbow"), dict(kind=0), dict(spots=[100.0, -1.0]), dict(spots=[100.0, math.nan]), dict(spots=100.0),
               dict(spots=[100.0]), dict(spots=[100.0] * 9, sigmas=[0.2] * 9), dict(spots=[], sigmas=[]),
               dict(sigmas=[0.2, 0.0]), dict(sigmas=[0.2, math.inf]), dict(weights=[0.5, -0.5]), dict(weights=[1.0]),
               dict(weights=[0.5, math.nan]), dict(dividend_yields=[0.0, math.inf]), dict(dividend_yields=[0.0]),
               dict(correlation=[[1.0, 0.5]]), dict(correlation=np.eye(3)), dict(correlation=[[1.0, 1.5], [1.5, 1.0]]),
               dict(correlation=[[1.0, 0.5], [0.4, 1.0]]), dict(correlation=[[1.0, math.nan], [math.nan, 1.0]]),
               dict(spots=[100.0, 95.0, 90.0], sigmas=[0.2] * 3, correlation=npd),
               dict(option_type="straddle"), dict(K=-1.0), dict(T=0.0), dict(r=-0.01), dict(n_steps=0), dict(n_paths=0),
               dict(n_paths=1)):
        with pytest.raises(ValueError):
            price_american_basket(**{**base, **kw})
    for kind in KINDS:
        with pytest.raises(AssertionError):  # a valid call gets as far as the device
            price_american_basket(**base, kind=kind)


# ------------------------------------------------------------------ the restatement itself
def test_restatement_with_identity_correlation_is_the_oracles_gbm_per_asset():
    S0, sig, q, w, _ = CASES[2]
    r, T, N, M, seed, stream, off = 0.05, 1.0, 37, 2_000, 11, 4, 321
    L, a, b, _, _ = br.table(S0, sig, q, w, np.eye(3), "basket", r, T, N)
    z = [orc.gbm_normals(M // 2, N, seed, stream, off + (k << 40)) for k in range(3)]
    A = br.assets(z, S0, a, b, L)
    for k in range(3):
        ref = orc.gbm_paths(M, N, S0[k], r - q[k], sig[k], T, seed, stream, off + (k << 40)).astype(np.float64)
        assert np.abs(A[k] / ref - 1.0).max() <= 2e-5, k
    # a correlated factor leaves asset 0 alone and moves the others
    L2 = br.table(S0, sig, q, w, CASES[2][4], "basket", r, T, N)[0]
    A2 = br.assets(z, S0, a, b, L2)
    assert np.array_equal(A2[0], A[0]) and not np.allclose(A2[1], A[1], rtol=1e-3)
    # the sample correlation of the log-returns is rho (P N = 37,000 samples: 4 / sqrt(n) = 0.021)
    lr = np.diff(np.log(A2[:, :, :M // 2]), axis=1).reshape(3, -1)
    assert np.abs(np.corrcoef(lr) - CASES[2][4]).max() <= 0.021


def test_index_rules_of_the_restatement():
    A = np.array([[[100.0, 50.0]], [[80.0, 90.0]], [[120.0, 10.0]]], np.float32)
    w = [0.5, 1.0, 0.25]
    assert np.array_equal(br.index(A, w, "basket"), [[160.0, 117.5]])
    assert np.array_equal(br.index(A, w, "best-of"), [[80.0, 90.0]]) and np.array_equal(br.index(A, w, "worst-of"), [[30.0, 2.5]])
    g = br.index(A, [0.5, 0.25, 0.25], "geometric", S0=[100.0, 80.0, 120.0], G0=math.sqrt(100.0) * 80.0 ** 0.25 * 120.0 ** 0.25)
    assert g[0, 0] == pytest.approx(math.sqrt(100.0) * 80.0 ** 0.25 * 120.0 ** 0.25, rel=1e-6)
    assert g[0, 1] == pytest.approx(math.sqrt(50.0) * 90.0 ** 0.25 * 10.0 ** 0.25, rel=1e-6)
    for kind in KINDS:  # one asset of weight 1 is its own index
        one = br.index(A[:1], [1.0], kind, S0=[100.0], G0=100.0)
        assert np.allclose(one, A[0], rtol=1e-12)


# ------------------------------------------------------------------ the C example
def test_c_example_compiles_and_links(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    exe = tmp_path / "american_basket"
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "american_basket.c"), "-o", str(exe), "-L", os.path.dirname(lib), "-lomc",
           "-lm", "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.run(cmd, check=True)
    assert exe.exists()

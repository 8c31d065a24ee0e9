"""Jump-diffusion without a GPU (include/omc.h "jump-diffusion"): the new symbols and struct
layouts, the host-side table of omc_jump_table against its restatement (tests/helpers/jump_ref.py) bit for bit, every
refusal code, the ValueErrors of price_american_jumps, the restatement's own count rule and Merton series, and the C
example."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import dividend_ref as dr
from helpers import jump_ref as jr
from options_model_amd import _build, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO24 = 1 << 24


def _params(T=1.0, N=16, **kw):
    kw.setdefault("semantics", "two_pass")
    return _ffi.make_params(n_paths=1000, n_steps=N, T=T, **kw)


# ------------------------------------------------------------------ ABI
def test_symbols_structs_and_version():
    lib = _ffi.load_library()
    for s in ("omc_jump_table", "omc_price_american_jump"):
        assert hasattr(lib, s) and s in _ffi.SIGNATURES
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert C.sizeof(_ffi.Jump) == 24
    assert C.sizeof(_ffi.JumpResult) == C.sizeof(_ffi.Result) + 32
    assert _ffi.JumpResult.base.offset == 0 and _ffi.JumpResult.ms_jump_paths.offset == C.sizeof(_ffi.Result)
    assert _ffi.JumpResult.n_thresholds.offset == C.sizeof(_ffi.Result) + 24
    import options_model_amd
    assert callable(options_model_amd.price_american_jumps) and options_model_amd.JumpResult is not None


def test_struct_layouts_match_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "omc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(omc_jump), offsetof(omc_jump, mu_j), offsetof(omc_jump, sigma_j),\n'
                   '         sizeof(omc_jump_result), offsetof(omc_jump_result, ms_jump_paths), offsetof(omc_jump_result, kappa),\n'
                   '         offsetof(omc_jump_result, drift_rate), offsetof(omc_jump_result, n_thresholds));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    J, R = _ffi.Jump, _ffi.JumpResult
    assert got == [C.sizeof(J), J.mu_j.offset, J.sigma_j.offset, C.sizeof(R), R.ms_jump_paths.offset, R.kappa.offset,
                   R.drift_rate.offset, R.n_thresholds.offset]


# ------------------------------------------------------------------ the table
# x = lambda T / n_steps -> (entries below 2^24, the leading thresholds).  Only these x: on another one the C library's
# exp and the restatement's could differ in the last place and move a threshold by one.
TABLES = [(0.0, 0, []),
          (0.004, 2, [16710241, 16777082]),
          (1.0 / 16.0, 4, [15760736, 16745782, 16776565, 16777206]),
          (0.25, 6, [13066109, 16332636, 16740952, 16774978, 16777105, 16777211]),
          (1.0, 10, [6171993, 12343986, 15429982])]


@pytest.mark.parametrize("x,n_thr,lead", TABLES)
def test_table_matches_the_restatement_bit_for_bit(x, n_thr, lead):
    T, N = 1.0, 16
    lam, mu, sj, r, q = x * N / T, -0.1, 0.15, 0.05, 0.02
    assert lam * T / N == x
    thr, kappa, rate = _ffi.jump_table(_params(T, N, r=r), (lam, mu, sj), q)
    rthr, rk, rr, rn = jr.table(lam, mu, sj, r, q, T, N)
    assert thr.dtype == np.uint32 and np.array_equal(thr, rthr)
    assert kappa == pytest.approx(rk, rel=1e-15) and rate == pytest.approx(rr, rel=1e-15)
    assert kappa == pytest.approx(math.exp(mu + 0.5 * sj * sj) - 1.0, rel=1e-15)
    assert rate == pytest.approx((r - q) - lam * kappa, rel=1e-15)
    assert int((thr < TWO24).sum()) == rn == n_thr
    assert list(thr[:len(lead)]) == lead
    assert np.all(thr[n_thr:] == TWO24) and np.all(np.diff(thr.astype(np.int64)) >= 0)
    if x == 0.0:  # exp(-0) = 1: no word reaches thr[0], no step ever jumps (and the pricing delegates)
        assert np.all(thr == TWO24)


def test_table_outputs_may_be_null():
    lib = _ffi.load_library()
    p, j = _params(), _ffi.Jump(2.0, -0.1, 0.15)
    assert lib.omc_jump_table(C.byref(p), C.byref(j), 0.0, None, None, None) == 0
    k = C.c_double()
    assert lib.omc_jump_table(C.byref(p), C.byref(j), 0.0, None, C.byref(k), None) == 0
    assert k.value == pytest.approx(math.exp(-0.1 + 0.01125) - 1.0, rel=1e-15)


# ------------------------------------------------------------------ refusals
def _rc(p, j, q=0.0):
    lib = _ffi.load_library()
    return lib.omc_jump_table(C.byref(p) if p is not None else None, C.byref(j) if j is not None else None, q, None, None, None)


def test_every_invalid_input_returns_its_code():
    ok, J = _params(), _ffi.Jump
    assert _rc(ok, J(1.0, -0.1, 0.15), 0.02) == 0 and _rc(ok, J(0.0, 0.0, 0.0), -0.02) == 0
    assert _rc(None, J(1.0, 0.0, 0.0)) == -7
    assert _rc(ok, None) == -25
    for q in (math.nan, math.inf, -math.inf):
        assert _rc(ok, J(1.0, 0.0, 0.0), q) == -17
    for lam in (-1e-9, math.nan, math.inf, -math.inf):
        assert _rc(ok, J(lam, 0.0, 0.0)) == -26, lam
    for mu in (math.nan, math.inf, -math.inf):
        assert _rc(ok, J(1.0, mu, 0.1)) == -27, mu
    for sj in (-1e-9, math.nan, math.inf):
        assert _rc(ok, J(1.0, 0.0, sj)) == -27, sj
    assert _rc(ok, J(16.0, 0.0, 0.0)) == 0  # x = 1 exactly is accepted
    assert _rc(ok, J(16.0000001, 0.0, 0.0)) == -28 and _rc(_params(T=2.0), J(9.0, 0.0, 0.0)) == -28
    assert _rc(_params(antithetic=False), J(1.0, 0.0, 0.0)) == -24
    for sem in ("reference", "textbook"):
        assert _rc(_params(semantics=sem), J(1.0, 0.0, 0.0)) == -11
    # the omc_params checks of omc_price_american
    j = J(1.0, 0.0, 0.0)
    assert _rc(_params(S0=-1.0), j) == -1 and _rc(_params(r=-0.01), j) == -2
    assert _rc(_params(N=0), j) == -3 and _rc(_params(N=5000), j) == -8
    assert _rc(_params(sigma=0.0), j) == -5
    # the pricing call refuses a null context and a null result before anything else
    lib = _ffi.load_library()
    out = _ffi.JumpResult()
    assert lib.omc_price_american_jump(None, C.byref(ok), C.byref(j), 0.0, C.byref(out), None, 0) == -7
    # the Python binding raises ValueError for every one of them
    for bad in ((-1.0, 0.0, 0.0), (1.0, math.nan, 0.0), (1.0, 0.0, -0.5), (17.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            _ffi.jump_table(ok, bad)
    with pytest.raises(ValueError):
        _ffi.jump_table(ok, (1.0, 0.0, 0.0), math.nan)


def test_facade_refuses_bad_arguments_before_any_device_work(monkeypatch):
    from options_model_amd import price_american_jumps

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks")
    monkeypatch.setattr(_ffi, "default_context", no_device)
    base = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=4096, n_steps=20, jump_intensity=1.0)
    for kw in (dict(jump_intensity=-1.0), dict(jump_intensity=math.nan), dict(jump_intensity=math.inf),
               dict(jump_mean=math.nan), dict(jump_mean=math.inf), dict(jump_vol=-0.1), dict(jump_vol=math.nan),
               dict(dividend_yield=math.inf), dict(jump_intensity=20.5), dict(model="sabr"), dict(option_type="straddle"),
               dict(S0=-1.0), dict(n_steps=0), dict(n_paths=0), dict(sigma=None)):
        with pytest.raises(ValueError):
            price_american_jumps(**{**base, **kw})
    with pytest.raises(AssertionError):  # a valid call gets as far as the device
        price_american_jumps(**base)


# ------------------------------------------------------------------ the restatement itself
def test_count_rule_on_hand_made_words():
    thr = np.array([10, 20, 30] + [TWO24] * 13, np.uint32)
    assert list(jr.count([0, 9, 10, 19, 20, 29, 30, TWO24 - 1], thr)) == [0, 0, 1, 1, 2, 2, 3, 3]
    # equal thresholds count together; a threshold of 2^24 is never reached by a 24-bit word
    assert int(jr.count(5, np.array([5, 5, 5] + [TWO24] * 13, np.uint32))) == 3
    assert int(jr.count(TWO24 - 1, np.full(16, TWO24, np.uint32))) == 0
    assert int(jr.count(TWO24 - 1, np.full(16, TWO24 - 1, np.uint32))) == 16
    # the table at x = 1: the words at the thresholds themselves
    thr = jr.table(16.0, 0.0, 0.0, 0.05, 0.0, 1.0, 16)[0]
    assert [int(jr.count(int(t), thr)) for t in thr[:10]] == list(range(1, 11))
    assert [int(jr.count(int(t) - 1, thr)) for t in thr[:10]] == list(range(0, 10))


def test_draws_use_the_stated_counters_and_words():
    """a fake Philox that returns its own counter: word (t-1) & 3 of block (t-1) >> 2 decides step t; the size block of
    step t is 0xC0000000 | t"""
    seen = []

    def fake(ctr, key):
        seen.append(tuple(int(c) for c in ctr))
        assert key == (0x89ABCDEF, 0x01234567)
        if ctr[2] & 0x80000000:
            return np.array([TWO24 << 7, 0, 0, 0], np.uint32)  # u1 = (2^23 + 0.5) / 2^24, u2 = 0
        cb = ctr[2] & 0xFFFF
        return np.array([(100 * (4 * cb + i + 1)) << 8 for i in range(4)], np.uint32)  # step t -> w = 100 t
    thr = np.array([250, 550] + [TWO24] * 14, np.uint32)
    n, z = jr.draws(fake, 1, 6, 0x0123456789ABCDEF, 7, (5 << 32) | 9, thr)
    assert list(n[:, 0]) == [0, 0, 0, 1, 1, 1, 2]
    assert seen[:2] == [(9, 5, 0x40000000, 7), (9, 5, 0x40000001, 7)]
    assert seen[2:] == [(9, 5, 0xC0000000 | t, 7) for t in (3, 4, 5, 6)]
    u1 = ((1 << 23) + 0.5) / TWO24
    assert np.all(z[3:, 0] == math.sqrt(-2.0 * math.log(u1))) and np.all(z[:3, 0] == 0.0)
    assert list(jr.first_jump_step(n)) == [3] and list(jr.first_jump_step(np.zeros((7, 2), np.int64))) == [7, 7]


def test_apply_without_jumps_returns_the_vanilla_matrix():
    rng = np.random.default_rng(5)
    V = np.cumprod(np.exp(0.05 * rng.standard_normal((9, 8))), axis=0).astype(np.float32)
    n, z = np.zeros((9, 4), np.int64), np.zeros((9, 4))
    assert np.array_equal(jr.apply(V, n, z, -0.1, 0.15).astype(np.float32), V)
    n[3, 1], z[3, 1] = 2, 0.5
    S = jr.apply(V, n, z, -0.1, 0.15)
    f = math.exp(2 * -0.1 + math.sqrt(2.0) * 0.15 * 0.5)
    assert np.allclose(S[3:, 1] / V[3:, 1], f, rtol=1e-12) and np.allclose(S[3:, 5] / V[3:, 5], f, rtol=1e-12)  # both partners
    keep = [0, 2, 3, 4, 6, 7]
    assert np.array_equal(S[:, keep].astype(np.float32), V[:, keep]) and np.array_equal(S[:3].astype(np.float32), V[:3])


def test_merton_series():
    S0, K, r, q, sig, T = 100.0, 95.0, 0.03, 0.02, 0.3, 1.0  # (lambda T <= 16: the mass beyond 60 terms is below 1e-16)
    for is_put in (True, False):  # lambda = 0: Black-Scholes-Merton
        # (equal up to sqrt(sigma^2), which need not round back to sigma)
        assert jr.merton(S0, K, r, q, sig, T, 0.0, -0.1, 0.15, is_put) == pytest.approx(dr.bsm(S0, K, r, q, sig, T, is_put), rel=1e-14)
    for lam, mu, sj in ((1.0, -0.1, 0.15), (8.0, -0.05, 0.1), (16.0, 0.02, 0.05)):  # put-call parity
        c, p = (jr.merton(S0, K, r, q, sig, T, lam, mu, sj, False), jr.merton(S0, K, r, q, sig, T, lam, mu, sj, True))
        assert c - p == pytest.approx(S0 * math.exp(-q * T) - K * math.exp(-r * T), rel=1e-12)
        assert c > dr.bsm(S0, K, r, q, sig, T, False)  # jumps add variance


# ------------------------------------------------------------------ the C example
def test_c_example_compiles_and_links(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    exe = tmp_path / "american_jumps"
    cmd = ["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "american_jumps.c"), "-o", str(exe), "-L", os.path.dirname(lib), "-lomc",
           "-lm", "-Wl,-rpath," + os.path.dirname(lib)]
    subprocess.run(cmd, check=True)
    assert exe.exists()

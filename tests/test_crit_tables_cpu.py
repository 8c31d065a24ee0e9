"""Pass 2's exercise-table builder (options_model_amd/csrc/omc_crit.h) compiled for the host: on adversarial fits its
intervals must decide every spot as the float64 predicate does -- checked ordinal by ordinal around every endpoint and
candidate, and on a spread of the whole non-negative float range -- or the step must be reported irregular."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "options_model_amd", "csrc")
TOP = 0x7F800000


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("crit") / "crit_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++20", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "helpers", "crit_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    d, u32p, u8p = C.c_double, np.ctypeslib.ndpointer(np.uint32), np.ctypeslib.ndpointer(np.uint8)
    lib.crit_host_build.argtypes = [C.c_int, C.c_int, d, d, d, d, d, u32p]
    lib.crit_host_build.restype = C.c_int
    lib.crit_host_eval.argtypes = [C.c_int, C.c_int, d, d, d, d, d, u32p, u32p, C.c_int64, u8p, u8p]
    return lib


def _ord(x):
    return int(np.array(x, np.float32).view(np.uint32)) if x < 3.4e38 else TOP


def _check(lib, kind, is_put, K, ck, b0, b1, b2, extra=()):
    tab = np.zeros(4, np.uint32)
    ok = lib.crit_host_build(kind, is_put, K, ck, b0, b1, b2, tab)
    if not ok:
        return None
    pts = [0, 1, TOP - 1, TOP]
    for o in (tab[0], tab[1], tab[0] + tab[2], tab[1] + tab[3]):
        pts.append(int(o))
    for s in (K, ck, *extra):
        if s > 0:
            pts.append(_ord(s))
    rng = np.random.default_rng(kind * 7 + is_put)
    near = np.concatenate([np.arange(max(p - 300, 0), min(p + 300, TOP) + 1, dtype=np.int64) for p in pts])
    bits = np.unique(np.concatenate([near, np.linspace(0, TOP, 200_001).astype(np.int64),
                                     rng.integers(0, TOP + 1, 200_000)])).astype(np.uint32)
    pred, tbl = np.zeros(bits.size, np.uint8), np.zeros(bits.size, np.uint8)
    lib.crit_host_eval(kind, is_put, K, ck, b0, b1, b2, tab, bits, bits.size, pred, tbl)
    bad = np.flatnonzero(pred != tbl)
    assert bad.size == 0, (kind, is_put, b0, b1, b2, tab, bits[bad[:8]])
    return tab, int(pred.sum())


INF = float("inf")
FITS = [
    # (b0, b1, b2): typical, no fit, linear, concave (two intervals), roots outside the float32 range
    (2.0, -40.0, 150.0),
    (INF, 0.0, 0.0),
    (1.5, -30.0, 0.0),
    (0.5, 0.0, 0.0),
    (-3.0, 10.0, -400.0),
    (-1.0, -150.0, -900.0),
    (1e30, 0.0, 1e-40),
    (-1e-30, 0.0, 0.0),
    (0.0, -100.0, 1e-300),
    (5.0, -200.0, 1e6),
]


@pytest.mark.parametrize("kind", [0, 1], ids=["stored", "partner"])
@pytest.mark.parametrize("is_put", [1, 0], ids=["put", "call"])
@pytest.mark.parametrize("fit", FITS, ids=[str(i) for i in range(len(FITS))])
def test_tables_match_predicate(lib, kind, is_put, fit):
    out = _check(lib, kind, is_put, 100.0, 97.3, *fit)
    if fit == (INF, 0.0, 0.0):
        assert out is not None and out[1] == 0  # no fit: never exercises, and that is certified


def test_two_intervals_come_out(lib):
    """put, stored path: pay(u) - cont(u) = -(b2 u^2 + (b1 + K) u + b0).  With b2 u^2 + (b1 + K) u + b0 = -100 (u + 0.3)
    (u + 0.1) the path exercises for u < -0.3 and for -0.1 < u < 0: spots below 70 and between 90 and 100."""
    K = 100.0
    b2, b1, b0 = -100.0, -40.0 - K, -3.0
    out = _check(lib, 0, 1, K, 97.3, b0, b1, b2)
    assert out is not None
    tab = out[0]
    assert tab[2] > 0 and tab[3] > 0
    lo = sorted(((int(tab[0]), int(tab[2])), (int(tab[1]), int(tab[3]))))
    f = lambda o: float(np.array(o, np.uint32).view(np.float32))  # noqa: E731
    assert lo[0][0] == 0 and abs(f(lo[0][0] + lo[0][1]) - 70.0) < 1e-4  # [0, 70)
    assert abs(f(lo[1][0]) - 90.0) < 1e-4 and abs(f(lo[1][0] + lo[1][1]) - 100.0) < 1e-4  # (90, 100)


def test_nearly_flat_linear_fit_is_irregular(lib):
    """b2 = 0 and b1 within rounding of -K (put): the sign of pay - cont is rounding noise over a wide stretch"""
    tab = np.zeros(4, np.uint32)
    assert lib.crit_host_build(0, 1, 100.0, 97.3, 1e-3, -100.0 * (1 + 1e-13), 0.0, tab) == 0
    assert lib.crit_host_build(1, 0, 100.0, 97.3, 1e-3, 100.0 * (1 - 1e-13), 0.0, tab) == 0


def test_tangent_roots_are_irregular(lib):
    """a double root of pay - cont: no certified switch, the step falls back to the float64 decisions"""
    K = 100.0
    # put stored: -(b2 u^2 + (b1 + K) u + b0) has a double root at u0 when b1 + K = -2 b2 u0, b0 = b2 u0^2
    b2, u0 = 50.0, -0.1
    b1, b0 = -2 * b2 * u0 - K, b2 * u0 * u0
    tab = np.zeros(4, np.uint32)
    assert lib.crit_host_build(0, 1, K, 97.3, b0, b1, b2, tab) == 0


def test_nonfinite_fits_are_irregular(lib):
    tab = np.zeros(4, np.uint32)
    assert lib.crit_host_build(0, 1, 100.0, 97.3, float("nan"), 0.0, 0.0, tab) == 0
    assert lib.crit_host_build(1, 0, 100.0, 97.3, 1.0, INF, 0.0, tab) == 0


def test_random_fits(lib):
    rng = np.random.default_rng(5)
    irregular = 0
    for _ in range(60):
        b2 = float(rng.choice([0.0, 1.0]) * rng.normal(0, 300))
        fit = (float(rng.normal(2, 3)), float(rng.normal(-50, 60)), b2)
        for kind in (0, 1):
            for is_put in (0, 1):
                if _check(lib, kind, is_put, 100.0, float(rng.uniform(60, 140)), *fit) is None:
                    irregular += 1
    assert irregular <= 4

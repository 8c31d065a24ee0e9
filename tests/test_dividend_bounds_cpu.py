"""What omc_price_american_bounds_div and omc_dividend_paths_f32 offer without a GPU: the symbols, the
header and the ABI version, the facade's argument checks, the host tables of a call against a plain-Python restatement, the
fuzz cases, the conditions the directed GPU cases of tests/test_gpu_dividend_bounds.py must meet on their INPUTS, the
absorbing-zero case on float64 paths, and the known answers the GPU statistics are held against, cross-checked here."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import bounds_ref as br
from helpers import call_catalogue as cat
from helpers import dividend_bounds_case as dc
from helpers import dividend_bounds_catalogue as dcat
from helpers import dividend_known as dk
from helpers import dividend_ref as dr
from options_model_amd import _build, _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_symbols_header_and_abi_version():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    names = ["omc_dividend_paths_f32", "omc_price_american_bounds_div"]
    assert sorted(_ffi.DIVIDEND_BOUNDS_SIGNATURES) == names
    assert not set(_ffi.DIVIDEND_BOUNDS_SIGNATURES) & (set(_ffi.SIGNATURES) | set(_ffi.JUMP_BOUNDS_SIGNATURES))
    for name, n_args in zip(names, (9, 11)):
        assert len(_ffi.DIVIDEND_BOUNDS_SIGNATURES[name][1]) == n_args
        assert len(getattr(lib, name).argtypes) == n_args  # exported and bound
    header = open(os.path.join(ROOT, "include", "omc_dividend_bounds.h")).read()
    assert '#include "omc.h"' in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(omc_[a-z0-9_]+)\s*\(", code))) == names
    assert re.search(r"\bint omc_dividend_paths_f32\(omc_ctx\* ctx, const omc_params\* p, double q, const omc_dividend\* d, "
                     r"int n_div,\s*int step_offset, float\* S, float\* V", header)
    assert re.search(r"\bint omc_price_american_bounds_div\(omc_ctx\* ctx, const omc_params\* p, double q, "
                     r"const omc_dividend\* d, int n_div,\s*const omc_bounds_config\* cfg", header)
    omc_h = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert re.search(r"#define OMC_ABI_VERSION 14\b", omc_h)
    # the new error code is the first free one below the lowest that omc.h uses
    assert "Error -40" in omc_h and not re.search(r"(?<![\w.])-4[1-9]\b", omc_h)
    assert "-41 step_offset" in header


@pytest.mark.parametrize("kw,match", [
    (dict(control_variate=True), "control_variate"), (dict(suboptimality_check="european"), "european"),
    (dict(suboptimality_check="lattice"), "suboptimality_check"),
    (dict(suboptimality_check="payoff", exercise_every=2), "exercise_every"),
    (dict(model="Heston", heston_scheme="calibrator"), "heston_scheme"), (dict(model="Heston", heston_scheme="qe"), "heston_scheme"),
    (dict(model="Heston", heston_scheme="milstein"), "heston_scheme"),
    (dict(dividends=[(0.5,)]), "a dividend is"), (dict(dividends=[(0.5, 1.0, "stock")]), "kind"),
    (dict(dividends=[(0.0, 1.0)]), "time"), (dict(dividends=[(1.5, 1.0)]), "time"), (dict(dividends=[(0.5, -1.0)]), "amount"),
    (dict(dividends=[(0.5, 1.0, "proportional")]), "proportional"), (dict(dividend_yield=float("nan")), "dividend"),
    (dict(n_inner=255), "n_inner"), (dict(policy="given"), "betas"), (dict(betas=np.zeros((5, 4))), "betas"),
    (dict(policy="lattice"), "policy"), (dict(model="SABR"), "model"), (dict(option_type="straddle"), "option_type")],
    ids=["control-variate", "european", "check", "check-and-schedule", "calibrator", "qe", "scheme", "item", "kind", "time-0",
         "time-late", "negative", "proportional-1", "yield", "odd-inner", "given-no-betas", "betas-not-given", "policy", "model",
         "option-type"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_american_bounds_dividends

    args = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, dividends=[(0.4, 1.0)], device=10 ** 6)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_american_bounds_dividends(**args)


def test_facade_is_exported():
    import options_model_amd as oma

    assert callable(oma.price_american_bounds_dividends) and issubclass(oma.DividendBoundsResult, oma.BoundsResult)
    fields = oma.DividendBoundsResult.__dataclass_fields__
    assert {"dividend_yield", "n_div_steps", "first_div_step"} <= set(fields)


def test_the_catalogue_calls_every_symbol_of_the_extension_header():
    """tests/test_call_catalogue_cpu.py's rule for the table of the extension header: every symbol is called by an entry of
    tests/helpers/dividend_bounds_catalogue.py, every entry makes a call of its family, every family has two size classes and
    draws at (seed, stream, pair_offset) -- so tests/test_gpu_dividend_bounds_calls.py leaves none of them out"""
    used = dcat.symbols_used()
    called = set().union(*used.values())
    assert set(_ffi.DIVIDEND_BOUNDS_SIGNATURES) <= called
    plumbing = {"omc_alloc", "omc_free", "omc_memcpy_h2d", "omc_memcpy_d2h", "omc_set_option"}
    for e in dcat.CATALOGUE:
        work = used[e.name] - plumbing
        assert work == {"omc_" + e.family + ("_f32" if e.family == "dividend_paths" else "")}, (e.name, work)
        assert e.name == f"{e.family}/{e.name.split('/')[1]}/{e.cls}"
    assert len({e.name for e in dcat.CATALOGUE}) == len(dcat.CATALOGUE)
    for fam in dcat.FAMILIES:
        assert {e.cls for e in dcat.CATALOGUE if e.family == fam} == {"S", "M"}
    assert sorted(dcat.DRAWING) == dcat.FAMILIES and not set(dcat.FAMILIES) & set(cat.FAMILIES)


def test_the_catalogue_entries_follow_the_key_sweep():
    """call_catalogue.drawing reaches the (seed, stream, pair_offset) of every entry's omc_params"""
    class ArgLib(cat.RecordingLib):
        def __init__(self):
            super().__init__()
            self.params = []

        def __getattr__(self, name):
            fn = super().__getattr__(name)

            def noting(*args):
                self.params += [a._obj for a in args if isinstance(getattr(a, "_obj", None), _ffi.Params)]
                return fn(*args)
            return noting

    for e in dcat.CATALOGUE:
        ctx = cat.recording_context()
        ctx.lib = ArgLib()
        try:
            with cat.drawing(0x9E3779B97F4A7C15, 0xDEADBEEF, (1 << 32) - 3):
                e.call(ctx)
        finally:
            ctx.handle = None
        assert ctx.lib.params, e.name
        for p in ctx.lib.params:
            assert p.seed == 0x9E3779B97F4A7C15 and p.pair_offset == (1 << 32) - 3 and 0 <= p.stream - 0xDEADBEEF < 16, e.name


# ------------------------------------------------------------------ the host tables
NEVER = 0x7000


def tables_ref(mul, cash, has, off):
    """the restatement: the entries behind `off` with their steps counted from it and the gap to the next, the closing entry,
    and for every date t the packed word (index of the first entry with step > t) << 16 | steps until it"""
    N = len(has) - 1
    ent = [[k - off, float(mul[k]), float(cash[k]), 0] for k in range(off + 1, N + 1) if has[k]]
    for a, b in zip(ent, ent[1:]):
        a[3] = b[0] - a[0]
    if ent:
        ent[-1][3] = NEVER
    first = []
    for t in range(N + 1):
        after = [j for j, e in enumerate(ent) if e[0] > t]
        first.append((after[0] << 16 | ent[after[0]][0] - t) if after else (len(ent) << 16 | NEVER))
    return ent + [[0x7fffffff, 1.0, 0.0, 0]], first


@pytest.fixture(scope="module")
def tables_exe(tmp_path_factory):
    """a stand-alone host program around dividend_tables of the private header csrc/omc_dividend_bounds.h: it reads N, the
    offset and N + 1 rows (has, mul, cash) and prints the table and first_after"""
    cxx = shutil.which("g++") or shutil.which("c++")
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_build._hipcc()))), "include")
    if cxx is None or not os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
        pytest.skip("no host C++ compiler or no HIP headers")
    d = tmp_path_factory.mktemp("divtab")
    src = d / "main.cpp"
    src.write_text('#include <cstdio>\n#include "omc_dividend_bounds.h"\n'
                   "int main() {\n  int N, off;\n  if (scanf(\"%d %d\", &N, &off) != 2) return 1;\n"
                   "  std::vector<float> mul(N + 1), cash(N + 1);\n  std::vector<int32_t> has(N + 1);\n"
                   "  for (int k = 0; k <= N; ++k) if (scanf(\"%d %a %a\", &has[k], &mul[k], &cash[k]) != 3) return 1;\n"
                   "  std::vector<omc::DivEntry> tab;\n  std::vector<omc::DivStart> first;\n"
                   "  omc::dividend_tables(N, mul.data(), cash.data(), has.data(), off, &tab, &first);\n"
                   "  printf(\"%zu\\n\", tab.size());\n"
                   "  for (auto& e : tab) printf(\"%d %a %a %d\\n\", e.step, e.mul, e.cash, e.pad);\n"
                   "  for (auto f : first) printf(\"%u\\n\", f);\n  return 0;\n}\n")
    exe = d / "divtab"
    subprocess.run([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-I", _build.CSRC, str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


def _tables(exe, mul, cash, has, off):
    N = len(has) - 1
    text = f"{N} {off}\n" + "".join(f"{int(h)} {float(m).hex()} {float(c).hex()}\n" for h, m, c in zip(has, mul, cash))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    n = int(out[0])
    ent = [[int(a), float.fromhex(b), float.fromhex(c), int(d)] for a, b, c, d in (ln.split() for ln in out[1:n + 1])]
    return ent, [int(x) for x in out[n + 1:n + 2 + N]]


def _schedules():
    """omc_dividend_schedule's edge cases and 200 random schedules -> (T, N, dividends)"""
    yield 1.0, 1, []
    yield 1.0, 1, [(1.0, 2.0, "cash")]
    yield 1.0, 4, [(1e-12, 1.0, "cash"), (1.0, 1.0, "cash")]                      # clamped to step 1; on step N
    yield 1.0, 4, [(0.25, 1.0, "cash"), (0.25 + 1e-12, 0.1, "proportional")]     # on a grid date and just behind it
    yield 2.0, 8, [(0.5, 1.0, "cash"), (0.5, 0.5, "proportional"), (0.5, 2.0, "cash")]  # three on one step, order kept
    yield 1.0, 13, [(k / 13.0, 0.5, "cash") for k in range(1, 14)]               # every step
    yield 1.0, 9, [(0.95, 0.0, "cash")]                                            # an amount of 0 is an entry
    rng = np.random.default_rng(29)
    for _ in range(200):
        N, T = int(rng.integers(1, 40)), float(rng.uniform(0.25, 3.0))
        yield T, N, [(float(rng.uniform(1e-6, 1.0)) * T, float(rng.uniform(0.0, 5.0)), "cash") if rng.integers(0, 2) else
                     (float(rng.uniform(1e-6, 1.0)) * T, float(rng.uniform(0.0, 0.2)), "proportional")
                     for _ in range(int(rng.integers(0, 7)))]


def test_host_tables_equal_their_restatement(tables_exe):
    n = 0
    for T, N, divs in _schedules():
        p = _ffi.make_params(is_put=True, semantics="two_pass", n_paths=2, n_steps=N, S0=100.0, K=100.0, r=0.05, sigma=0.2, T=T,
                             seed=1)
        mul, cash, has = _ffi.dividend_schedule(p, 0.0, divs)
        m2, c2, h2 = dr.schedule(T, N, divs)  # (the library's table is the restatement's)
        assert np.array_equal(mul, m2) and np.array_equal(cash, c2) and np.array_equal(has, h2)
        for off in range(N + 1):
            ent, first = _tables(tables_exe, mul, cash, has, off)
            ref_ent, _ = tables_ref(mul, cash, has, off)
            assert ent == ref_ent, (T, N, divs, off)
            if off == 0:
                assert first == tables_ref(mul, cash, has, 0)[1], (T, N, divs)
            n += 1
        # what the kernels rely on: a word's countdown is in 1 .. N - t or NEVER, its index is in bounds, NEVER outlasts any path
        for t, f in enumerate(first_all := tables_ref(mul, cash, has, 0)[1]):
            ix, cd = f >> 16, f & 0xffff
            assert 0 <= ix <= int(has.sum()) and (cd == NEVER if ix == int(has.sum()) else 1 <= cd <= N - t)
        assert NEVER > 4094 and len(first_all) == N + 1
    assert n > 2000


# ------------------------------------------------------------------ the cases
def test_fuzz_cases_are_deterministic_and_cover_the_space():
    a, b = dc.fuzz_cases(8), dc.fuzz_cases(8)
    assert a == b and dc.fuzz_cases(9)[:8] == a
    assert {c["model"] for c in a} == set(dc.MODELS) and {c["policy"] for c in a} == set(dc.POLICIES)
    assert [bool(c["every"]) for c in a] == [i % 3 == 1 for i in range(8)]
    assert [c["check"] for c in a] == ["payoff" if i % 3 == 2 else None for i in range(8)]
    assert all(0 <= len(c["divs"]) <= 5 and all(1 <= k <= c["N"] for k, _, _ in c["divs"]) for c in a)
    assert any(c["refill"] for c in a) and {c["n_inner"] for c in a} == set(dc.N_INNER)
    many = dc.fuzz_cases(64)
    assert {len(c["divs"]) for c in many} == set(range(6))
    assert {kind for c in many for _, _, kind in c["divs"]} == {"cash", "proportional"}


def test_dividends_of_a_case_land_on_their_steps():
    for c in dc.DIRECTED + dc.fuzz_cases(16):
        _, _, has = dr.schedule(c["T"], c["N"], dc.dividends_of(c))
        assert sorted(np.flatnonzero(has)) == dc.steps_of(c)


def test_directed_cases_cover_the_issue_list():
    D = dc.DIRECTED
    assert 12 <= len(D) <= 14
    assert {c["N"] for c in D} >= {1, 2, 4, 5, 9, 13} and {c["n_inner"] for c in D} == {2, 64, 130, 200}
    assert {c["n_outer"] for c in D} == {2, 6, 40} and {c["is_put"] for c in D} == {True, False}
    assert {c["policy"] for c in D} == set(dc.POLICIES) and {c["q"] for c in D} == {0.0, 0.03}
    assert {c["model"] for c in D} == set(dc.MODELS) and any(c["irr_every"] for c in D)
    kinds = [{kind for _, _, kind in c["divs"]} for c in D]
    assert {"cash"} in kinds and {"proportional"} in kinds and {"cash", "proportional"} in kinds
    steps = [dc.steps_of(c) for c in D]
    assert any(1 in s for s in steps) and any(c["N"] in s for c, s in zip(D, steps))  # a dividend on step 1 and one on step N
    assert any(len(c["divs"]) > len(s) for c, s in zip(D, steps))  # two dividends on one step
    assert any(b - a == 1 for s in steps for a, b in zip(s, s[1:]))  # two on adjacent steps
    # both sides of a Philox block boundary: 4 | 5 under GBM, 2 | 3 under Heston
    assert any(c["model"] == "gbm" and {4, 5} <= set(s) for c, s in zip(D, steps))
    assert any(c["model"] != "gbm" and {2, 3} <= set(s) for c, s in zip(D, steps))
    for m in dc.MODELS:
        mine = [(c, s) for c, s in zip(D, steps) if c["model"] == m]
        # an item date t equal to a dividend step (the entry must not be applied again): a dividend step below N
        assert any(k < c["N"] for c, s in mine for k in s), m
        # an item date one before a dividend step: the first inner step has the dividend (every step k >= 1 has date k - 1)
        assert any(s for _, s in mine), m
        # no entry after some t: the last dividend step is below N
        assert any(s and s[-1] < c["N"] for c, s in mine), m
    assert len(dc.ABSORBING) == 2 and all(c in D for c in dc.ABSORBING)


@pytest.mark.parametrize("c", dc.ABSORBING, ids=[dc.case_id(c) for c in dc.ABSORBING])
def test_the_large_dividend_takes_some_columns_to_zero(c):
    """on float64 paths of the case's law (under Heston: lognormal steps at sqrt(v0), close enough for a count): between 1 % and
    50 % of the columns are at 0 from the dividend step on"""
    rng = np.random.default_rng(5)
    N, T, M = c["N"], c["T"], 20_000
    sig = c["sigma"] if c["model"] == "gbm" else math.sqrt(c["hp"]["v0"])
    dt = T / N
    z = rng.standard_normal((N, M))
    V = np.vstack([np.full(M, c["S0"]), c["S0"] * np.exp(np.cumsum((c["r"] - c["q"] - 0.5 * sig * sig) * dt
                                                                       + sig * math.sqrt(dt) * z, axis=0))])
    S = dr.apply(V, *dr.schedule(T, N, dc.dividends_of(c)))
    k0 = min(dc.steps_of(c))
    zero = S[k0] == 0.0
    assert 0.01 < zero.mean() < 0.5, zero.mean()
    assert np.all(S[k0:, zero] == 0.0) and np.all(S[:k0] > 0.0)


# ------------------------------------------------------------------ the known answers
def test_european_with_proportional_dividends_is_black_scholes_at_the_scaled_spot():
    """(a), cross-checked by quadrature over the terminal lognormal and against the project's closed forms"""
    S0, K, r, q, sig, T, deltas = 100.0, 100.0, 0.05, 0.03, 0.2, 1.0, [0.02, 0.03, 0.01]
    def terminal(x):
        return S0 * np.prod([1 - d for d in deltas]) * np.exp((r - q - 0.5 * sig * sig) * T + sig * math.sqrt(T) * x)

    for is_put in (True, False):
        v = dk.european_proportional(S0, K, r, q, sig, T, deltas, is_put)
        quad = math.exp(-r * T) * dk.normal_mean(lambda x: np.maximum(K - terminal(x) if is_put else terminal(x) - K, 0.0))
        assert abs(v - quad) < 1e-7 * K, (v, quad)
        assert abs(v - dr.bsm(S0 * float(np.prod([1 - d for d in deltas])), K, r, q, sig, T, is_put)) < 1e-10
    assert abs(dk.european_proportional(S0, K, r, 0.0, sig, T, [], True) - br.black_scholes(S0, K, r, sig, T, True)) < 1e-10


@pytest.mark.parametrize("N,k,delta,S0", [(8, 5, 0.06, 100.0), (6, 2, 0.03, 105.0), (12, 12, 0.08, 95.0)])
def test_call_with_one_proportional_dividend_against_the_lattice(N, k, delta, S0):
    """(b) against a recombining lattice restricted to the grid dates; the margin is the lattice's own resolution difference"""
    K, r, sig, T = 100.0, 0.05, 0.2, 1.0
    v = dk.bermudan_call_one_proportional(S0, K, r, sig, T, N, k, delta)
    assert abs(v - dk.bermudan_call_one_proportional(S0, K, r, sig, T, N, k, delta, n=40_001)) < 1e-7
    m = 60
    a, b = (dk.lattice_call_one_proportional(S0, K, r, sig, T, N, k, delta, mm) for mm in (m, 2 * m))
    assert abs(b - v) <= abs(b - a) + 1e-9, (v, a, b)
    # the dividend matters: the value lies above the European call on the scaled spot and below the dividend-free call
    assert dk.european_proportional(S0, K, r, 0.0, sig, T, [delta], False) < v < br.black_scholes(S0, K, r, sig, T, False)
    # with delta = 0 early exercise is worthless: the dividend-free European call
    v0 = dk.bermudan_call_one_proportional(S0, K, r, sig, T, N, k, 0.0)
    assert abs(v0 - br.black_scholes(S0, K, r, sig, T, False)) < 1e-9


def test_backward_induction_against_the_quadrature_and_the_lattice():
    """(c): the log-spot grid's value with the dividend made proportional against (b), and without a dividend against the
    project's lattice value on the grid dates; the margin is the induction's own grid-doubling difference"""
    S0, K, r, sig, T, N, k = 100.0, 100.0, 0.05, 0.2, 1.0, 6, 3
    a, b = (dk.bermudan_one_dividend_grid(S0, K, r, sig, T, N, k, 0.06, "proportional", False, m=m, nz=nz)
            for m, nz in ((1500, 1201), (3000, 2401)))
    assert abs(b - dk.bermudan_call_one_proportional(S0, K, r, sig, T, N, k, 0.06)) <= abs(b - a)
    a, b = (dk.bermudan_one_dividend_grid(S0, K, r, sig, T, N, k, 0.0, "cash", True, m=m, nz=nz)
            for m, nz in ((1500, 1201), (3000, 2401)))
    assert abs(b - br.lattice(S0, K, r, sig, T, N, True)) <= abs(b - a)
    # a cash dividend lowers the call and raises the put
    assert dk.bermudan_one_dividend_grid(S0, K, r, sig, T, N, k, 4.0, "cash", True) > a

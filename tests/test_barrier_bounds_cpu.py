"""What omc_price_american_bounds_barrier and omc_barrier_paths_state_f32 offer without a GPU: the
symbols, the header and the ABI version, the facade's argument checks, the call catalogue, the conditions the directed GPU
cases of tests/test_gpu_barrier_bounds.py must meet on their INPUTS (asserted on the C oracle's paths at the cases' own Philox
coordinates), the fuzz cases, the restatement of tests/helpers/barrier_bounds_ref.py against bounds_ref where the barrier is
out of reach, and hand-computed answers at N = 1 and N = 2."""
import math
import os
import re

import numpy as np
import pytest

from helpers import barrier_bounds_case as bc
from helpers import barrier_bounds_catalogue as bcat
from helpers import barrier_bounds_ref as bbr
from helpers import barrier_ref as bar
from helpers import bounds_check_ref as bcr
from helpers import bounds_ref as br
from helpers import bounds_schedule_ref as bsr
from helpers import call_catalogue as cat
from options_model_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the interface
def test_symbols_header_and_abi_version():
    lib = _ffi.load_library()
    assert lib.omc_abi_version() == 14 == _ffi.ABI_VERSION
    assert len(_ffi.SIGNATURES) == 80
    names = ["omc_barrier_paths_state_f32", "omc_price_american_bounds_barrier"]
    assert sorted(_ffi.BARRIER_BOUNDS_SIGNATURES) == names
    assert not set(_ffi.BARRIER_BOUNDS_SIGNATURES) & (set(_ffi.SIGNATURES) | set(_ffi.JUMP_BOUNDS_SIGNATURES)
                                                      | set(_ffi.DIVIDEND_BOUNDS_SIGNATURES))
    for name, n_args in zip(names, (9, 9)):
        assert len(_ffi.BARRIER_BOUNDS_SIGNATURES[name][1]) == n_args
        assert len(getattr(lib, name).argtypes) == n_args  # exported and bound
    header = open(os.path.join(ROOT, "include", "omc_barrier_bounds.h")).read()
    assert '#include "omc.h"' in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(omc_[a-z0-9_]+)\s*\(", code))) == names
    assert re.search(r"\bint omc_barrier_paths_state_f32\(omc_ctx\* ctx, const omc_params\* p, const omc_barrier\* b, "
                     r"int start_hit, float\* E, float\* S,\s*float\* V", header)
    assert re.search(r"\bint omc_price_american_bounds_barrier\(omc_ctx\* ctx, const omc_params\* p, const omc_barrier\* b,\s*"
                     r"const omc_bounds_config\* cfg", header)
    omc_h = open(os.path.join(ROOT, "include", "omc.h")).read()
    assert re.search(r"#define OMC_ABI_VERSION 14\b", omc_h)


@pytest.mark.parametrize("kw,match", [
    (dict(control_variate=True), "control_variate"), (dict(suboptimality_check="european"), "european"),
    (dict(suboptimality_check="lattice"), "suboptimality_check"),
    (dict(suboptimality_check="payoff", exercise_every=2), "exercise_every"), (dict(monitoring="continuous"), "monitoring"),
    (dict(model="Heston", heston_scheme="calibrator"), "heston_scheme"), (dict(model="Heston", heston_scheme="qe"), "heston_scheme"),
    (dict(model="Heston", heston_scheme="milstein"), "heston_scheme"), (dict(barrier_type="down-and-up"), "barrier_type"),
    (dict(barrier=0.0), "barrier H"), (dict(barrier=float("nan")), "barrier H"), (dict(barrier=100.0), "already knocked"),
    (dict(barrier=101.0), "already knocked"), (dict(barrier=99.0, barrier_type="up-and-in"), "already knocked"),
    (dict(n_inner=255), "n_inner"), (dict(policy="given"), "betas"), (dict(betas=np.zeros((5, 4))), "betas"),
    (dict(policy="given", betas=np.zeros((4, 4))), "shape"), (dict(policy="lattice"), "policy"), (dict(model="SABR"), "model"),
    (dict(option_type="straddle"), "option_type")],
    ids=["control-variate", "european", "check", "check-and-schedule", "continuous", "calibrator", "qe", "scheme", "kind", "H-0",
         "H-nan", "on-the-barrier", "beyond-down", "beyond-up", "odd-inner", "given-no-betas", "betas-not-given", "betas-shape",
         "policy", "model", "option-type"])
def test_facade_refuses_before_the_device(kw, match):
    """no context is given and none is made (device 10^6 does not exist): the checks come first"""
    from options_model_amd import price_barrier_bounds

    args = dict(S0=100.0, K=100.0, r=0.05, sigma=0.2, T=1.0, n_paths=1000, n_steps=4, barrier=90.0, device=10 ** 6)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        price_barrier_bounds(**args)


def test_facade_is_exported_with_the_defaults_of_price_american_bounds():
    import inspect

    import options_model_amd as oma

    assert callable(oma.price_barrier_bounds) and issubclass(oma.BarrierBoundsResult, oma.BoundsResult)
    assert {"barrier", "barrier_type", "monitoring", "model"} <= set(oma.BarrierBoundsResult.__dataclass_fields__)
    mine, base = (inspect.signature(f).parameters for f in (oma.price_barrier_bounds, oma.price_american_bounds))
    for name in ("option_type", "policy", "n_lower", "n_outer", "n_inner", "seed", "stream", "betas", "exercise_every", "ctx"):
        assert mine[name].default == base[name].default, name
    assert mine["barrier_type"].default == "down-and-out" and mine["model"].default == "GBM"
    assert mine["heston_scheme"].default == "reference" and mine["suboptimality_check"].default is None


def test_the_catalogue_calls_every_symbol_of_the_extension_header():
    used = bcat.symbols_used()
    called = set().union(*used.values())
    assert set(_ffi.BARRIER_BOUNDS_SIGNATURES) <= called
    plumbing = {"omc_alloc", "omc_free", "omc_memcpy_h2d", "omc_memcpy_d2h", "omc_set_option"}
    for e in bcat.CATALOGUE:
        work = used[e.name] - plumbing
        assert work == {"omc_" + e.family + ("_f32" if e.family == "barrier_paths_state" else "")}, (e.name, work)
        assert e.name == f"{e.family}/{e.name.split('/')[1]}/{e.cls}"
    assert len({e.name for e in bcat.CATALOGUE}) == len(bcat.CATALOGUE)
    for fam in bcat.FAMILIES:
        assert {e.cls for e in bcat.CATALOGUE if e.family == fam} == {"S", "M"}
    assert sorted(bcat.DRAWING) == bcat.FAMILIES and not set(bcat.FAMILIES) & set(cat.FAMILIES)


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

    for e in bcat.CATALOGUE:
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


# ------------------------------------------------------------------ the cases
def test_directed_cases_cover_the_issue_list():
    C, S = bc.CASES, bc.SHAPES
    assert len(C) == 84 and len({bc.case_id(c) for c in C}) == len(C)
    full = {(c["shape"], c["kind"], c["is_put"], c["mode"]) for c in C if c["shape"] in bc.FULL}
    assert len(full) == 3 * 4 * 2 * 3  # all four kinds x put / call x GBM and Heston 0 / 1 x plain / scheduled / payoff
    assert {S[n]["model"] for n in bc.FULL} == set(bc.MODELS)
    assert {s["N"] for s in S.values()} == {1, 2, 3, 7, 13} and {s["n_inner"] for s in S.values()} == {2, 64, 130, 200}
    for s in S.values():
        assert s["n_outer"] % 2 == 0 and s["n_outer"] <= 40 and s["n_lower"] <= 1400 and s["M"] <= 4096
    assert any(s["n_outer"] % 4 for s in S.values())  # ragged: no multiple of a wave, some no multiple of four
    assert {c["policy"] for c in C} == set(bc.POLICIES)
    for name in bc.SIDE:
        mine = [c for c in C if c["shape"] == name]
        assert len(mine) == 4 and {c["is_put"] for c in mine} == {True, False}
    assert all(bbr.knock_out(c["kind"]) for c in C if S[c["shape"]]["N"] == 1)  # (N = 1 has no item that starts hit)


@pytest.mark.parametrize("name", list(bc.SHAPES))
@pytest.mark.parametrize("side", ["down", "up"])
def test_every_shape_and_barrier_meets_the_four_conditions(name, side):
    """on the C oracle's paths at the shape's own seed and streams: (a) between 10 % and 90 % of the outer paths hit; (b) some
    outer path is first hit at step 1 and some at step N; (c) the first wave of some item holds lanes (pairs) with a partner
    knocked and lanes with none -- with n_inner = 2 there is one lane, and the condition is on its two partners; (d) for the
    knock-ins some item starts un-hit (every t = 0 item does) and some starts hit (an outer path hit before N)"""
    s = bc.SHAPES[name]
    N, kind = s["N"], side + "-and-out"
    H = bc.barrier_of(s, kind)
    hs = bar.discrete_hit_steps(bc.oracle_outer(s), kind, H)
    assert 0.1 <= np.mean(hs <= N) <= 0.9, np.mean(hs <= N)
    assert (hs == 1).any() and (hs == N).any()
    P = s["n_inner"] // 2
    mixed = False
    for i in range(s["n_outer"]):
        h = bar.discrete_hit_steps(bc.oracle_item0(s, i), kind, H) <= N
        w = (h[:P] | h[P:])[:64]
        mixed = bool(h[0] != h[1]) if P == 1 else bool(w.any() and not w.all())
        if mixed:
            break
    assert mixed
    uses_knock_in = any(c["shape"] == name and not bbr.knock_out(c["kind"]) for c in bc.CASES)
    assert not uses_knock_in or (hs <= N - 1).any()


def test_fuzz_cases_are_deterministic_and_cover_the_space():
    a, b = bc.fuzz_cases(8), bc.fuzz_cases(8)
    assert a == b and bc.fuzz_cases(9)[:8] == a
    assert {c["model"] for c in a} == set(bc.MODELS) and {c["policy"] for c in a} == set(bc.POLICIES)
    assert {c["kind"] for c in a} == set(bc.KINDS)
    assert [bool(c["every"]) for c in a] == [i % 3 == 1 for i in range(8)]
    assert [c["check"] for c in a] == ["payoff" if i % 3 == 2 else None for i in range(8)]
    assert any(c["refill"] for c in a) and {c["n_inner"] for c in a} == set(bc.N_INNER)
    for c in bc.fuzz_cases(64):
        assert (c["H"] < c["S0"]) == c["kind"].startswith("down") and 0.02 <= abs(c["H"] / c["S0"] - 1.0) <= 0.10
        assert c["n_outer"] % 2 == 0 and 2 <= c["n_outer"] <= 40 and c["n_lower"] <= 1400 and c["M"] <= 4096


# ------------------------------------------------------------------ the restatement
def _paths(rng, rows, m, s0, sig=0.25, dt=0.1):
    z = rng.standard_normal((rows - 1, m // 2))
    z = np.concatenate([z, -z], axis=1)
    x = np.cumsum(-0.5 * sig * sig * dt + sig * math.sqrt(dt) * z, axis=0)
    return np.concatenate([np.full((1, m), s0), s0 * np.exp(x)]).astype(np.float32)


def _table(rng, N):
    t = np.zeros((N + 1, 4))
    t[1:, 0], t[1:, 1], t[1:, 2], t[1:, 3] = 4.0 + rng.random(N), -40.0, 60.0, 50.0
    return t


@pytest.mark.parametrize("is_put", [True, False])
@pytest.mark.parametrize("k,check", [(0, None), (3, None), (0, "payoff")])
def test_restatement_with_an_unreachable_barrier_is_bounds_ref(is_put, k, check):
    """a knock-out no path reaches: the lower bound, Q^, the step count and the samples of bounds_ref / bounds_schedule_ref /
    bounds_check_ref on the same paths; a knock-in no path reaches: nothing"""
    rng = np.random.default_rng(7)
    N, n_outer, n_inner, K, r, T = 7, 6, 8, 100.0, 0.05, 0.7
    So, Sl = _paths(rng, N + 1, n_outer, 100.0), _paths(rng, N + 1, 400, 100.0)
    items = {(i, t): _paths(rng, N - t + 1, n_inner, float(So[t, i])) for i in range(n_outer) for t in range(N)}
    inner = lambda i, t: items[(i, t)]  # noqa: E731
    betas = _table(rng, N)
    if not is_put:
        betas[:, :3] *= 0.5
    for kind in ("down-and-out", "up-and-out"):
        H = bc.unreachable(kind)
        lo = bbr.lower_bound(Sl, kind, H, K, r, T, is_put, betas, k)
        up = bbr.upper_bound(So, inner, kind, H, K, r, T, is_put, betas, k, check)
        ref_lo = bsr.lower_bound(Sl, K, r, T, is_put, betas, k)
        if k >= 2:
            ref = bsr.upper_bound(So, inner, K, r, T, is_put, betas, k)
        elif check:
            ref = bcr.upper_bound(So, inner, 1, K, r, T, is_put, betas)
        else:
            ref = br.upper_bound(So, inner, K, r, T, is_put, betas)
        assert (lo["lower"], lo["se_lower"], lo["n_exercised"]) == (ref_lo["lower"], ref_lo["se_lower"], ref_lo["n_exercised"])
        assert lo["n_exercised"] > 0
        np.testing.assert_array_equal(up["q"], ref["q"])
        assert up["inner_path_steps"] == ref["inner_path_steps"] and np.all(up["hit"] == 0)
        # (the walk over the kept dates with every date kept adds the same terms in the same order as the dense walk)
        np.testing.assert_allclose(up["samples"], ref["samples"], rtol=1e-13, atol=1e-13 * K)
    for kind in ("down-and-in", "up-and-in"):
        H = bc.unreachable(kind)
        lo = bbr.lower_bound(Sl, kind, H, K, r, T, is_put, betas, k)
        up = bbr.upper_bound(So, inner, kind, H, K, r, T, is_put, betas, k, check)
        assert (lo["lower"], lo["se_lower"], lo["n_exercised"]) == (0.0, 0.0, 0)
        assert (up["upper"], up["se_upper"]) == (0.0, 0.0) and np.all(up["q"] == 0.0)


def test_known_answer_one_date():
    """N = 1, K = 100, H = 90 (down), r = 0, put.  Lower paths end at 95, 85, 105, 89.5: hit are 85 and 89.5.
    knock-out: payoffs 5, 0 (dead), 0, 0 (dead) -> pair means (5 + 0) / 2 and (0 + 0) / 2 -> lower 1.25
    knock-in:  payoffs 0 (never live), 15, 0, 10.5 -> pair means 0, 12.75 -> lower 6.375"""
    S = np.array([[100.0] * 4, [95.0, 85.0, 105.0, 89.5]], np.float32)  # pairs (0, 2) and (1, 3)
    betas = np.zeros((2, 4))
    out = bbr.lower_bound(S, "down-and-out", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert out["lower"] == 1.25 and out["n_exercised"] == 0 and out["ties"] == 0
    assert out["se_lower"] == math.sqrt((2.5 * 2.5 / 2 - 1.25 * 1.25) / 2)
    inn = bbr.lower_bound(S, "down-and-in", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert inn["lower"] == 6.375
    # in + out = the vanilla one-date value on the same paths
    assert inn["lower"] + out["lower"] == br.lower_bound(S, 100.0, 0.0, 1.0, True, betas)["lower"] == 7.625
    # the upper bound of a one-date game is its Q^_0 sample: max over t = 1 of Z_1 - (Z_1 - Q^_0) = Q^_0
    So = np.array([[100.0, 100.0], [95.0, 85.0]], np.float32)
    inner = lambda i, t: S  # noqa: E731
    up = bbr.upper_bound(So, inner, "down-and-out", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert np.all(up["q"] == 1.25) and np.all(up["samples"] == 1.25) and up["inner_path_steps"] == 2 * 4
    assert list(up["hit"]) == [0, 1] and up["keep"].all()  # (both t = 0 items are live: column 1 is hit at step 1 > 0)


def test_known_answer_two_dates():
    """N = 2, K = 100, H = 90 (down), r = 0, put, a policy that exercises at date 1 exactly where the payoff exceeds 4.
        column   row 1   row 2    knock-out                              knock-in
        0        95      80       exercises at 1: 5                      dead at 1; hit at 2, live: 20
        1        97      85       3 < 4 continues; hit at 2: stops, 0    hit at 2, live at N: 15
        2        88      99       hit at 1: stops at 1 with 0            live from 1: 12 > 4, exercises: 12
        3        99      96       continues, at N: 4                     never live: 0
    pairs (0, 2), (1, 3): knock-out means 2.5, 2 -> 2.25; knock-in means 16, 7.5 -> 11.75.  Stopped before N: knock-out
    columns 0 and 2 (an exercise and a knock), knock-in column 2."""
    S = np.array([[100.0] * 4, [95.0, 97.0, 88.0, 99.0], [80.0, 85.0, 99.0, 96.0]], np.float32)
    betas = np.array([[0.0] * 4, [4.0, 0.0, 0.0, 10.0], [0.0] * 4])
    out = bbr.lower_bound(S, "down-and-out", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert (out["lower"], out["n_exercised"], out["ties"]) == (2.25, 2, 0)
    inn = bbr.lower_bound(S, "down-and-in", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert (inn["lower"], inn["n_exercised"]) == (11.75, 1)
    tau, Z, _ = bbr.first_stop(*bbr.encode(S, "down-and-out", 90.0, 100.0, True), "down-and-out", 0, 2, 100.0, 0.0, 1.0, True, betas)
    assert list(tau) == [1, 2, 1, 2] and list(Z) == [5.0, 0.0, 0.0, 4.0]
    # with exercise at date 2 only (k = 2) the knocked-out column 2 stops at date 2, not at its hit step: one step more
    tau, Z, _ = bbr.first_stop(*bbr.encode(S, "down-and-out", 90.0, 100.0, True), "down-and-out", 0, 2, 100.0, 0.0, 1.0, True, betas,
                               k=2)
    assert list(tau) == [2, 2, 2, 2] and list(Z) == [0.0, 0.0, 0.0, 4.0]
    # an item that starts hit: a knock-out's is dead (never simulated), a knock-in's is the vanilla game from there
    So = np.array([[100.0, 100.0], [88.0, 95.0], [99.0, 80.0]], np.float32)
    item = np.array([[88.0, 88.0], [99.0, 96.0]], np.float32)
    inner = lambda i, t: S if t == 0 else (item if i == 0 else np.array([[95.0, 95.0], [80.0, 97.0]], np.float32))  # noqa: E731
    ko = bbr.upper_bound(So, inner, "down-and-out", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert list(ko["hit"]) == [1, 2] and ko["q"][0, 1] == 0.0 and not ko["keep"][1, 0] and ko["keep"][1, 1]
    assert ko["q"][1, 1] == 1.5  # from 95 un-hit: 80 is hit at N -> 0, 97 -> 3
    assert ko["inner_path_steps"] == (1 + 2 + 1 + 2) * 2 + 2  # two t = 0 items, and the live t = 1 item's two paths
    ki = bbr.upper_bound(So, inner, "down-and-in", 90.0, 100.0, 0.0, 1.0, True, betas)
    assert ki["q"][0, 1] == 2.5 and ki["q"][1, 1] == 10.0  # from 88, hit: (1 + 4) / 2; from 95, un-hit: (20 + 0) / 2

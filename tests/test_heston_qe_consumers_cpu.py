"""The cases of tests/test_gpu_heston_qe_consumers.py (tests/helpers/heston_qe_cases.py) hold what the GPU tests rely on.  No GPU:
every case is restated in float64 (heston_qe_ref.paths) on the C oracle's normals, which are the device's, and the conditions
are asserted on the restatement alone -- a GPU test that compares the device with itself can then not pass empty.

  * barrier        tail levels: some paths hit and some do not, per direction, and no spot lies within relative 1e-3 of the
                   level (the device's float32 spots, 5e-5 away, then hit exactly where the restatement does).  Bulk levels
                   (n_paths >= 1000): at least 1 % of the paths pass the level by more than that margin, at least 1 % stay
                   more than the margin away
  * European       payoffs on both sides of the strike, puts and calls (n_paths > 2)
  * the three sets A: no exponential lane at any step.  C: every lane exponential at step 1.  B: a wave of 64 pairs with an
                   exponential and a quadratic lane at one step, wherever heston_qe_cases.expects_mixed says one can exist
  * jumps          cells with a jump and cells without; at 513 pairs x 7 steps both sides of the kernel's ballot hold
                   exponential lanes
  * dividends      no path is taken to 0 by the mixed schedule; the case that takes paths to 0 takes 1 % .. 50 % of them
"""
import numpy as np
import pytest

from helpers import dividend_ref as dr
from helpers import heston_qe_cases as qc
from helpers import heston_qe_ref as qe


# ---------------------------------------------------------------------------------------------- barrier
def barrier_conditions(case, S):
    """-> None, or the first condition the case misses"""
    M, N = case["M"], case["N"]
    for direction, H in zip(("down", "up"), case["tail"]):
        if not (H < qc.S0 if direction == "down" else H > qc.S0):
            return f"{direction} level {H} on the wrong side of S0"
        share = float((qc.hit_steps(S, direction, H) <= N).mean())
        if not 0.0 < share < 1.0:
            return f"{direction} {H}: hit share {share}"
        if qc.nearest_spot(S, H) <= qc.MARGIN:
            return f"{direction} {H}: a spot within {qc.nearest_spot(S, H):.2e}"
    if M >= 1000:
        for direction, H in zip(("down", "up"), qc.BULK):
            out, inside = (1.0 - qc.MARGIN, 1.0 + qc.MARGIN) if direction == "down" else (1.0 + qc.MARGIN, 1.0 - qc.MARGIN)
            clear_hit = float((qc.hit_steps(S, direction, H * out) <= N).mean())
            clear_miss = float((qc.hit_steps(S, direction, H * inside) > N).mean())
            if clear_hit < 0.01 or clear_miss < 0.01:
                return f"bulk {direction} {H}: {clear_hit} hit, {clear_miss} stay away"
    return None


@pytest.mark.parametrize("name", list(qc.barrier_cases()))
def test_barrier_levels_are_met_by_some_paths_and_touched_by_no_spot(name):
    c = qc.barrier_cases()[name]
    S = qc.restated(c["law"], c["M"], c["N"], c["seed"], c["stream"], c["off"])["S"]
    assert barrier_conditions(c, S) is None, name


def test_a_barrier_no_path_hits_is_noticed():
    """the check checked: the same case with its down level where no path goes"""
    c = dict(qc.BARRIER_ENCODE["enc-B-50"])
    S = qc.restated(c["law"], c["M"], c["N"], c["seed"], c["stream"], c["off"])["S"]
    assert barrier_conditions(c, S) is None
    c["tail"] = (1e-6 * qc.S0, c["tail"][1])
    assert "hit share 0.0" in barrier_conditions(c, S)


def test_barrier_cases_cover_the_lists_of_the_european_sums():
    import test_gpu_european_sums as es
    shapes = {(M, N) for N in es.BARRIER_N for M in es.BARRIER_M} | {es.BARRIER_BIG}
    for law in ("B", "C"):
        assert {(c["M"], c["N"]) for c in qc.BARRIER_EURO.values() if c["law"] == law} == shapes
    assert {(c["N"], c["M"]) for c in qc.BARRIER_ENCODE.values()} == {(50, 4096), (51, 4096)}
    assert all((c["M"], c["N"]) == (16384, 40) for c in qc.BARRIER_AMERICAN.values())
    assert all((c["M"], c["N"]) == (4096, 33) for c in qc.BARRIER_SHARD.values())


# ---------------------------------------------------------------------------------------------- European
def test_european_cases_have_payoffs_on_both_sides_of_the_strike():
    cases = qc.euro_cases()
    assert {law for law, *_ in cases} == {"A", "B", "C"}
    for law, M, N, stream in cases:
        ST = qc.restated(law, M, N, qc.EURO_SEED, stream, qc.EURO_OFFSET)["S"][-1]
        if M > 2:
            for is_put in (True, False):
                n_zero = int(np.count_nonzero((qc.K - ST if is_put else ST - qc.K) <= 0.0))
                assert 0 < n_zero < M, (law, M, N, stream, is_put, n_zero)


# ---------------------------------------------------------------------------------------------- the branches of each set
def test_every_set_takes_the_branches_it_is_for():
    seen = {}
    for label, law, M, N, seed, stream, off, rate, t in qc.set_cases():
        expo = qc.restated(law, M, N, seed, stream, off, rate, t)["expo"]
        what = (label, law, M, N, stream)
        if law == "A":
            assert not expo.any(), what
        elif law == "C":
            assert expo[0].all(), what
        else:
            mixed = bool(qc.mixed_waves(expo, M).any())
            if qc.expects_mixed(M, N):
                assert mixed, what
            seen.setdefault(label.split()[0], []).append(mixed)
    # every consumer has set B cases with a mixed wave
    for group in ("barrier", "european", "strikes", "surface", "dividends", "jumps", "batch", "chain", "sequence"):
        assert any(seen[group]), group


def test_step_one_takes_one_branch_in_every_lane():
    """what expects_mixed says of step 1, and the values its docstring quotes for set B"""
    for law in qc.LAWS:
        for N in (1, 5, 9, 50):
            expo = qc.restated(law, 2 * 257, N, qe.SEED, qe.STREAM)["expo"]
            assert expo[0].all() or not expo[0].any(), (law, N)
    for N, above in ((1, True), (5, True), (50, False)):
        c = qe.consts(qc.R, qc.T, N, *qc.law_args("B")[1:])
        m, s2 = qe.moments(np.array([qc.LAWS["B"]["v0"]]), c)
        assert (s2[0] / m[0] ** 2 > qe.PSI_C) == above, (N, s2[0] / m[0] ** 2)


# ---------------------------------------------------------------------------------------------- jumps
def test_jump_cases_have_cells_with_a_jump_and_cells_without():
    import test_gpu_dividends as gd
    import test_gpu_jumps as gj
    for M, N in gd.SHAPES[:4]:
        thr, _, rate = qc.jump_table(N, gj.lam_of(N), gj.MU, gj.SJ, gj.Q)
        for is_put, stream, off in qc.JUMP_COORDS:
            if not (is_put or M <= 5_000):  # the GPU test restates these coordinates only, as tests/test_gpu_jumps.py does
                continue
            n = qc.jump_counts(M, N, stream, off, tuple(int(x) for x in thr))[1:]
            assert (n > 0).any() and (n == 0).any(), (M, N, stream)
            if (M, N) != qc.BALLOT_SHAPE:
                continue
            assert qc.store_vec(M) == 1
            jumps = np.concatenate([n > 0, n > 0], axis=1)
            for law in qc.JUMP_LAWS:
                expo = qc.restated(law, M, N, qc.JUMP_SEED, stream, off, rate)["expo"]
                wave_jumps, wave_expo = qc.wave_any(jumps, M), qc.wave_any(expo, M)
                assert (wave_jumps & wave_expo).any(), (law, stream)    # the jump side of the ballot, exponential lanes in it
                assert (~wave_jumps & wave_expo).any(), (law, stream)   # the vanilla side


# ---------------------------------------------------------------------------------------------- dividends
def test_the_mixed_schedule_takes_no_path_to_zero_and_the_large_dividend_does():
    import test_gpu_dividends as gd
    for law in qc.DIV_LAWS:
        for M, N in gd.SHAPES:
            divs, steps = qc.mixed_schedule(N)
            p = gd.params("heston", qc.QE, M=M, N=N)
            assert (divs, steps) == gd.mixed_schedule(p, "heston")
            V = qc.restated(law, M, N, qc.DIV_SEED, qc.DIV_STREAM, 0, qc.R - qc.div_yield(law))["S"]
            S = dr.apply(V, *dr.schedule(qc.T, N, divs))
            assert S.min() > 0.0, (law, M, N)
        z = qc.DIV_ZERO
        V = qc.restated(law, z["M"], z["N"], z["seed"], z["stream"], 0, qc.R - z["q"])["S"]
        S = dr.apply(V, *dr.schedule(qc.T, z["N"], [((z["N"] // 2 - 0.5) * qc.T / z["N"], z["cash"][law], "cash")]))
        share = float((S[z["N"] // 2] == 0.0).mean())
        assert 0.01 <= share <= 0.50, (law, share)
        assert np.all(S[:z["N"] // 2] > 0.0)


# ---------------------------------------------------------------------------------------------- fuzz
def test_fuzz_laws_stay_within_the_sizes():
    cases = qc.fuzz_laws(6, 20270101)
    assert len(cases) == 6 and all(c["M"] <= 12_290 and 1 <= c["N"] <= 40 for c in cases)
    assert sum(c["xi"] ** 2 > 2.0 * c["kappa"] * c["theta"] for c in cases) == 2  # every third violates Feller

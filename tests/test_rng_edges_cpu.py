"""The mined edges of the random draws (tests/golden/rng_edges.json, tools/mine_rng_edges.py) hold what they claim, and the
references alone satisfy every condition tests/test_gpu_rng_edges.py puts on the device.  No GPU."""
import numpy as np
import pytest

from helpers import barrier_ref as br
from helpers import jump_ref as jr
from helpers import rng_edges as re_
from oracle import cpu as orc


@pytest.fixture(scope="module")
def fx():
    return re_.load()


def block_words(row):
    pair = row["pair"]
    return orc.philox4x32_10((pair & 0xFFFFFFFF, pair >> 32, row["c2"], re_.STREAM), (re_.SEED & 0xFFFFFFFF, re_.SEED >> 32)) >> 8


def test_bulk_words_are_the_scalar_function_row_for_row():
    for pair0, c2, stream, seed in ((0, 0, 0, 0), ((1 << 32) - 3, re_.COUNT_TAG | 3, re_.STREAM, re_.SEED),
                                    ((1 << 40) + 5, 0xC0000010, 1 << 31, (1 << 32) - 1), (123, re_.BRIDGE_TAG, 7, 1 << 63)):
        n = 70_001 if pair0 == 0 else 9  # above and below the size from which the loop runs in parallel
        W = orc.philox_words(n, pair0, c2, stream, seed)
        assert W.shape == (n, 4) and W.dtype == np.uint32
        for i in list(range(9)) + ([n - 1, n // 2] if n > 9 else []):
            g = pair0 + i
            assert np.array_equal(W[i], orc.philox4x32_10((g & 0xFFFFFFFF, g >> 32, c2, stream), (seed & 0xFFFFFFFF, seed >> 32)))
    # only the stream's low 32 bits enter the counter
    assert np.array_equal(orc.philox_words(4, 1, 2, re_.STREAM + (1 << 32), re_.SEED), orc.philox_words(4, 1, 2, re_.STREAM, re_.SEED))


def test_the_fixture_is_of_the_documented_scan(fx):
    assert (fx["seed"], fx["stream"], fx["n_pairs"], fx["n_blocks"], fx["n_steps"]) == \
        (re_.SEED, re_.STREAM, re_.N_PAIRS, re_.N_BLOCKS, re_.N_STEPS)
    assert fx["seed"] >> 32 and fx["stream"] >> 31  # both high halves are in play
    thr, _, _, n_thr = jr.table(re_.JUMP_LAM, -0.1, 0.15, 0.05, 0.02, re_.JUMP_T, re_.N_STEPS)  # thresholds: lambda T / N alone
    assert fx["jump_law"]["thr"] == [int(t) for t in thr] and fx["jump_law"]["n_thresholds"] == n_thr
    assert {r["class"] for r in fx["rows"]} == set(re_.CLASSES)
    assert 100 <= len(fx["rows"]) <= 1000


def test_every_class_has_at_least_eight_rows(fx):
    for cls in re_.CLASSES:
        assert len(re_.rows_of(fx, cls)) >= re_.MIN_ROWS, cls
    for v in re_.RADIUS_WORDS:
        assert any(r["words"][0] == v for r in re_.rows_of(fx, "radius")), hex(v)
    for v in re_.ANGLE_WORDS:
        assert any(r["words"][1] == v for r in re_.rows_of(fx, "angle")), hex(v)
    for v in re_.BRIDGE_WORDS:
        assert any(r["word"] == v for r in re_.rows_of(fx, "bridge")), hex(v)
    thr = fx["jump_law"]["thr"]
    for k in range(3):
        for v in (thr[k], thr[k] - 1):
            assert any(r["word"] == v for r in re_.rows_of(fx, "count_edge")), (k, v)


def test_every_row_rederives_from_philox_and_belongs_to_its_class(fx):
    thr = fx["jump_law"]["thr"]
    for r in fx["rows"]:
        assert 0 <= r["pair"] < re_.N_PAIRS
        w = block_words(r)
        cls = r["class"]
        if cls in ("radius", "angle", "tail"):
            assert 0 <= r["c2"] < re_.N_BLOCKS and r["slot"] in (0, 2)
            assert r["words"] == [int(w[r["slot"]]), int(w[r["slot"] + 1])], r
            if cls == "radius":
                assert r["words"][0] in re_.RADIUS_WORDS
            elif cls == "angle":
                assert r["words"][1] in re_.ANGLE_WORDS
            else:
                assert r["normal"] in (0, 1) and abs(re_.box_muller64(*r["words"])[r["normal"]]) > 5.2
        else:
            tag = re_.BRIDGE_TAG if cls == "bridge" else re_.COUNT_TAG
            assert r["c2"] & 0xC0000000 == tag and 0 <= (r["c2"] & 0x3FFFFFFF) < re_.N_BLOCKS and 0 <= r["slot"] < 4
            assert r["word"] == int(w[r["slot"]]), r
            assert r["step"] == 4 * (r["c2"] & 0x3FFFFFFF) + r["slot"] + 1
            if cls == "count_edge":
                assert r["word"] in (thr[r["k"]], thr[r["k"]] - 1) and r["k"] in (0, 1, 2)
            elif cls == "count_max":
                assert r["word"] >= thr[7]
            else:
                assert r["word"] in re_.BRIDGE_WORDS and r["columns"]
    tail = [abs(re_.box_muller64(*r["words"])[r["normal"]]) for r in re_.rows_of(fx, "tail")]
    assert len(tail) == re_.N_TAIL and tail == sorted(tail, reverse=True)


def test_the_oracles_normals_meet_the_contract_at_every_normal_row(fx):
    """what the GPU test asks of the device, asked of the C oracle's float32 normals: 4e-6 to the float64 Box-Muller on
    the fixture's words, finite, inside the largest possible |z|, and +-0 at radius word 0xFFFFFF"""
    worst = {}
    for r in re_.rows_of(fx, "radius", "angle", "tail"):
        Z = orc.gbm_normals(1, re_.N_STEPS, re_.SEED, re_.STREAM, r["pair"])[:, 0]
        assert np.all(np.isfinite(Z)) and np.abs(Z).max() <= re_.Z_MAX + re_.Z_TOL
        for t, z in re_.reference_normals(r).items():
            err = abs(float(Z[t]) - z)
            worst[r["class"]] = max(worst.get(r["class"], 0.0), err)
            assert err <= re_.Z_TOL, (r, t, float(Z[t]), z)
            if r["words"][0] == re_.W24:
                assert Z[t] == 0.0
    print({k: f"{v:.2e}" for k, v in worst.items()})
    assert abs(re_.box_muller64(0, 0)[0] - re_.Z_MAX) < 1e-7 and re_.box_muller64(re_.W24, 12345) == (0.0, 0.0)


def test_the_oracles_bulk_sample_has_next_to_no_normal_on_a_tail_threshold():
    """the bulk test of the GPU file sets aside values within 4e-6 of |z| = 3, 4, 4.5, 5 (at most 8): the oracle's own 2^24
    normals of that launch have one such value (at 3), so the allowance is not what makes the counts agree"""
    a = np.abs(orc.gbm_normals(1 << 20, re_.N_STEPS, re_.SEED, re_.STREAM, 0).astype(np.float64))
    near = [int((np.abs(a - t) <= re_.Z_TOL).sum()) for t in (3.0, 4.0, 4.5, 5.0)]
    print(near, [int((a > t).sum()) for t in (3.0, 4.0, 4.5, 5.0)])
    assert sum(near) <= 2 and (a > 5.0).sum() > 0


def test_the_counts_of_the_count_rows_are_what_the_class_says(fx):
    thr = np.array(fx["jump_law"]["thr"], np.uint32)
    for r in re_.rows_of(fx, "count_edge"):
        n = int(jr.count(r["word"], thr))
        assert n == r["count"] == (r["k"] + 1 if r["word"] == thr[r["k"]] else r["k"]), r
    top = re_.rows_of(fx, "count_max")
    assert len(top) == re_.N_MAX_COUNTS
    for r in top:
        assert int(jr.count(r["word"], thr)) == r["count"] >= 8, r
    # the restatement of the draws gives these counts at these cells
    for r in re_.rows_of(fx, "count_edge")[:6] + top[:2]:
        n, _ = jr.draws(orc.philox4x32_10, 1, re_.N_STEPS, re_.SEED, re_.STREAM, r["pair"], thr)
        assert n[r["step"], 0] == r["count"], r


def test_the_bridge_rows_are_decided_with_a_margin(fx):
    """no mined column can fall under the 1e-6 tie excuse of the barrier tests"""
    N = re_.N_STEPS
    for r in re_.rows_of(fx, "bridge"):
        Z = orc.gbm_normals(1, N, re_.SEED, re_.STREAM, r["pair"])
        u = br.bridge_uniforms(1, N, re_.SEED, re_.STREAM, r["pair"])
        V = orc.gbm_paths(2, N, re_.S0, re_.R, re_.SIG, re_.T, re_.SEED, re_.STREAM, r["pair"])
        assert int(round(float(u[r["step"] - 1, 0]) * 2 ** 24)) == r["word"]
        for H, c in r["columns"]:
            assert H in re_.BARRIERS and c in (0, 1)
            kind = "down-and-out" if H < re_.S0 else "up-and-out"
            hs, gap = br.continuous_hit_steps(V, Z, u, re_.S0, H, re_.R, re_.SIG, re_.T, kind)
            p = br.bridge_probabilities(Z, re_.S0, H, re_.R, re_.SIG, re_.T)[r["step"] - 1, c]
            assert gap[:, c].min() > re_.TIE_MARGIN
            assert br.discrete_hit_steps(V, kind, H)[c] > r["step"]  # the uniform decides, not the spot
            if r["word"] == re_.W24:
                assert p <= 1.0 - re_.P_MARGIN and hs[c] > r["step"]
            else:
                assert p >= re_.P_MARGIN and hs[c] == r["step"]

#!/usr/bin/env python3
"""Mine the counter space for the edge words of the random draws -> tests/golden/rng_edges.json.

The generators are counter-based (Philox4x32-10 on (pair lo, pair hi, third word, stream), key = seed lo / hi), so the
inputs no random sample reaches -- a radius word of 0 or 0xFFFFFF, an angle word on a quarter turn, a jump-count word
equal to a Poisson threshold, a bridge uniform of 0 -- can be found on the CPU and then asked of the device exactly,
through pair_offset.  This tool scans pairs 0 .. 2^25 at seed 0x9E3779B97F4A7C15, stream 0xDEADBEEF (both high halves
non-zero) with the C oracle's bulk words (oracle.cpu.philox_words):

  blocks 0..3                  radius / angle words of the normals, and the 32 largest |z| (float64 Box-Muller)
  0x40000000 | 0..3            jump-count words at lambda = 8, T = 1, N = 16: equal to thr[k] and thr[k] - 1, k = 0, 1, 2, and
                               the 16 rows with the largest counts
  0x80000000 | 0..3            bridge uniforms 0, 1 and 0xFFFFFF whose crossing test (tests/helpers/barrier_ref.py, GBM,
                               barriers 90 / 112) is unambiguous at that step

The classes and the row format are in tests/helpers/rng_edges.py.  Deterministic, no GPU, under a minute; running it again
reproduces the file byte for byte.  It fails if a class has fewer than 8 rows: enlarge the scan then, not the classes.

    python tools/mine_rng_edges.py [--out tests/golden/rng_edges.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import barrier_ref as br  # noqa: E402
from helpers import jump_ref as jr  # noqa: E402
from helpers import rng_edges as re_  # noqa: E402
from oracle import cpu as orc  # noqa: E402

CHUNK = 1 << 21


def scan(thr):
    """-> hits {name: list of (pair, block, slot, 24-bit words of the block)} over the three domains"""
    hits = {k: [] for k in ("radius", "angle", "small_radius", "count_edge", "count_max", "bridge")}
    edge_values = np.array(sorted({int(thr[k]) - d for k in range(3) for d in (0, 1)}), np.uint32)

    def keep(name, mask, W, p0, blk, slots):
        for i, j in zip(*np.nonzero(mask)):
            hits[name].append((p0 + int(i), blk, int(slots[j]), tuple(int(x) for x in W[i])))

    for p0 in range(0, re_.N_PAIRS, CHUNK):
        for blk in range(re_.N_BLOCKS):
            W = orc.philox_words(CHUNK, p0, blk, re_.STREAM, re_.SEED) >> 8
            rad, ang = W[:, 0::2], W[:, 1::2]
            keep("radius", ((rad + 3) & re_.W24) < 7, W, p0, blk, (0, 2))           # 0xFFFFFD .. 3
            keep("angle", ((ang + 1) & 0x3FFFFF) < 3, W, p0, blk, (1, 3))           # a quarter turn and its neighbours
            keep("small_radius", rad < 64, W, p0, blk, (0, 2))                      # |z| > 5 needs u1 < e^-12.5
            W = orc.philox_words(CHUNK, p0, re_.COUNT_TAG | blk, re_.STREAM, re_.SEED) >> 8
            keep("count_edge", np.isin(W, edge_values), W, p0, blk, (0, 1, 2, 3))
            keep("count_max", W >= thr[7], W, p0, blk, (0, 1, 2, 3))
            W = orc.philox_words(CHUNK, p0, re_.BRIDGE_TAG | blk, re_.STREAM, re_.SEED) >> 8
            keep("bridge", ((W + 1) & re_.W24) < 3, W, p0, blk, (0, 1, 2, 3))
    for v in hits.values():
        v.sort()  # (pair, block, slot) order
    return hits


def first_per_value(rows, value_of, values):
    out = []
    for v in values:
        out += [r for r in rows if value_of(r) == v][:re_.PER_VALUE]
    return sorted(out, key=lambda r: (r["pair"], r["c2"], r["slot"]))


def bridge_columns(pair, step, word):
    """the [barrier, partner] columns of a pair whose continuous-monitoring result is decided by the uniform of `step`,
    with a margin: no crossing before it, no spot crossing at it, p >= 1e-3 for the words 0 and 1 (a certain hit) or
    p <= 1 - 1e-3 for 0xFFFFFF (a certain miss), and no step of the column within 1e-5 of a tie"""
    N = re_.N_STEPS
    Z = orc.gbm_normals(1, N, re_.SEED, re_.STREAM, pair)
    u = br.bridge_uniforms(1, N, re_.SEED, re_.STREAM, pair)
    V = orc.gbm_paths(2, N, re_.S0, re_.R, re_.SIG, re_.T, re_.SEED, re_.STREAM, pair)
    cols = []
    for H in re_.BARRIERS:
        kind = "down-and-out" if H < re_.S0 else "up-and-out"
        prob = br.bridge_probabilities(Z, re_.S0, H, re_.R, re_.SIG, re_.T)
        hs, gap = br.continuous_hit_steps(V, Z, u, re_.S0, H, re_.R, re_.SIG, re_.T, kind)
        spot_hs = br.discrete_hit_steps(V, kind, H)
        near = np.abs(V[1:].astype(np.float64) / H - 1.0).min(axis=0) < 1e-3  # a spot the device could put on the other side
        for c in (0, 1):
            p = prob[step - 1, c]
            if gap[:, c].min() <= re_.TIE_MARGIN or near[c] or spot_hs[c] <= step:
                continue
            if word == re_.W24:
                ok = p <= 1.0 - re_.P_MARGIN and hs[c] > step
            else:
                ok = p >= re_.P_MARGIN and hs[c] == step
            if ok:
                cols.append([H, c])
    return cols


def mine():
    thr, _, _, n_thr = jr.table(re_.JUMP_LAM, 0.0, 0.0, 0.0, 0.0, re_.JUMP_T, re_.N_STEPS)
    thr = [int(t) for t in thr]
    hits = scan(thr)
    rows = []

    def normal_row(cls, h, slot):
        pair, blk, _, w = h
        return {"class": cls, "pair": pair, "c2": blk, "slot": slot, "words": [w[slot], w[slot + 1]]}

    rows += first_per_value([normal_row("radius", h, h[2]) for h in hits["radius"]], lambda r: r["words"][0], re_.RADIUS_WORDS)
    rows += first_per_value([normal_row("angle", h, h[2] - 1) for h in hits["angle"]], lambda r: r["words"][1], re_.ANGLE_WORDS)

    tail = []
    for h in hits["small_radius"]:
        r = normal_row("tail", h, h[2])
        for k, z in enumerate(re_.box_muller64(*r["words"])):
            tail.append((-abs(z), r["pair"], r["c2"], r["slot"], k, r))
    tail.sort(key=lambda t: t[:5])
    assert len(tail) >= re_.N_TAIL and -tail[re_.N_TAIL - 1][0] > 5.2, "enlarge the scan"
    rows += [dict(t[5], normal=t[4]) for t in tail[:re_.N_TAIL]]

    def count_row(cls, h):
        pair, blk, slot, w = h
        return {"class": cls, "pair": pair, "c2": re_.COUNT_TAG | blk, "slot": slot, "word": w[slot],
                "count": int(jr.count(w[slot], thr)), "step": 4 * blk + slot + 1}

    edge = []
    for h in hits["count_edge"]:
        r = count_row("count_edge", h)
        r["k"] = min(k for k in range(3) if r["word"] in (thr[k], thr[k] - 1))
        assert r["count"] == r["k"] + (r["word"] == thr[r["k"]])
        edge.append(r)
    rows += first_per_value(edge, lambda r: r["word"], [thr[k] - d for k in range(3) for d in (0, 1)])
    top = sorted((count_row("count_max", h) for h in hits["count_max"]), key=lambda r: (-r["count"], r["pair"], r["c2"], r["slot"]))
    assert len(top) >= re_.N_MAX_COUNTS and top[re_.N_MAX_COUNTS - 1]["count"] >= 8, "enlarge the scan"
    rows += top[:re_.N_MAX_COUNTS]

    bridge = []
    for pair, blk, slot, w in hits["bridge"]:
        step = 4 * blk + slot + 1
        cols = bridge_columns(pair, step, w[slot])
        if cols:
            bridge.append({"class": "bridge", "pair": pair, "c2": re_.BRIDGE_TAG | blk, "slot": slot, "word": w[slot],
                           "step": step, "columns": cols})
    rows += first_per_value(bridge, lambda r: r["word"], re_.BRIDGE_WORDS)

    for cls in re_.CLASSES:
        n = sum(r["class"] == cls for r in rows)
        assert n >= re_.MIN_ROWS, f"class {cls}: {n} rows -- enlarge the scan"
    return {"seed": re_.SEED, "stream": re_.STREAM, "n_pairs": re_.N_PAIRS, "n_blocks": re_.N_BLOCKS, "n_steps": re_.N_STEPS,
            "jump_law": {"lam": re_.JUMP_LAM, "T": re_.JUMP_T, "thr": thr, "n_thresholds": n_thr},
            "bridge_market": {"S0": re_.S0, "r": re_.R, "sigma": re_.SIG, "T": re_.T, "barriers": list(re_.BARRIERS)},
            "rows": rows}


def dump(fixture):
    """one row per line, keys in insertion order: stable bytes"""
    head = {k: v for k, v in fixture.items() if k != "rows"}
    lines = [json.dumps(head)[:-1] + ', "rows": [']
    lines += ["  " + json.dumps(r) + ("," if i + 1 < len(fixture["rows"]) else "") for i, r in enumerate(fixture["rows"])]
    return "\n".join(lines + ["]}"]) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=re_.PATH)
    args = ap.parse_args()
    fx = mine()
    with open(args.out, "w") as f:
        f.write(dump(fx))
    print({cls: sum(r["class"] == cls for r in fx["rows"]) for cls in re_.CLASSES}, "->", args.out)

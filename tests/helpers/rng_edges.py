"""The mined edges of the random draws (tests/golden/rng_edges.json, written by tools/mine_rng_edges.py).  TEST
INFRASTRUCTURE ONLY.

The generators are counter-based, so a word with probability 2^-24 is reached exactly: the tool scans the counter space
with the C oracle, keeps the coordinates (pair, third counter word, word slot) at which an edge word occurs, and the tests
ask the device for those pairs through pair_offset.  This module holds what the tool, the CPU test of the fixture and the
GPU tests share: the scan's constants, the class definitions and the float64 Box-Muller on box_muller's own u1, u2.

Row fields: `class`, `pair`, `c2` (the third counter word: block index, or tag | block), `slot` (word of the block),
and the 24-bit values: `words` = [radius, angle] for the normal classes (slot = 0 or 2, the radius word's), `word` for
the others.  Tail rows add `normal` (0: the cosine normal, 1: the sine normal); count rows `count`, `step` and, at a
threshold, `k`; bridge rows `step` and `columns` = [[barrier, partner], ...], the columns whose crossing test at that
step is unambiguous.
"""
import json
import math
import os

import numpy as np

SEED, STREAM = 0x9E3779B97F4A7C15, 0xDEADBEEF
N_PAIRS, N_BLOCKS, N_STEPS = 1 << 25, 4, 16
COUNT_TAG, BRIDGE_TAG = 0x40000000, 0x80000000
W24 = 0xFFFFFF

RADIUS_WORDS = (0, 1, 2, 3, 0xFFFFFD, 0xFFFFFE, 0xFFFFFF)
ANGLE_WORDS = (0, 1, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFF, 0x800000, 0x800001, 0xBFFFFF, 0xC00000, 0xC00001, 0xFFFFFF)
BRIDGE_WORDS = (0, 1, 0xFFFFFF)
PER_VALUE, N_TAIL, N_MAX_COUNTS, MIN_ROWS = 8, 32, 16, 8
CLASSES = ("radius", "angle", "tail", "count_edge", "count_max", "bridge")

# the jump law of the count rows (thresholds depend on lambda T / N alone) and the market of the bridge rows
JUMP_LAM, JUMP_T = 8.0, 1.0
S0, R, SIG, T = 100.0, 0.05, 0.2, 1.0
BARRIERS = (90.0, 112.0)  # down, up
P_MARGIN, TIE_MARGIN = 1e-3, 1e-5

Z_MAX = 5.8870502  # sqrt(-2 ln 2^-25): radius word 0
Z_TOL = 4e-6       # the normals' contract

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "rng_edges.json")


def load():
    with open(PATH) as f:
        return json.load(f)


def rows_of(fixture, *classes):
    return [r for r in fixture["rows"] if r["class"] in classes]


def box_muller64(radius24, angle24):
    """(z_cos, z_sin) in float64 from the two 24-bit words: u1, u2 exactly as box_muller forms them in float32 (u1 of
    word 0xFFFFFF rounds to 1.0), everything after that in float64"""
    u1 = np.float32(np.float32(radius24) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25))  # exact product: the fma's rounding
    u2 = np.float32(angle24) * np.float32(2.0 ** -24)
    rad = math.sqrt(-2.0 * math.log(float(u1))) if float(u1) < 1.0 else 0.0
    ang = 2.0 * math.pi * float(u2)
    return rad * math.cos(ang), rad * math.sin(ang)


def normal_steps(row):
    """the two steps (rows of a normals matrix, 0-based) a normal row's Box-Muller pair fills: block c2, words slot, slot+1"""
    t = 4 * row["c2"] + row["slot"]
    return t, t + 1


def reference_normals(row):
    """{step (0-based row of gbm_normals' matrix): float64 normal} of the row's Box-Muller pair"""
    zc, zs = box_muller64(*row["words"])
    t0, t1 = normal_steps(row)
    return {t0: zc, t1: zs}

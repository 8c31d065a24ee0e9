"""Record the bits of the Andersen-Broadie bound kernels' outputs for tests/test_gpu_bounds_bits.py.

Runs the cases of tests/helpers/bounds_bits_case.py -- one call per bound kernel -- with the library of the tree it is
started in and writes float.hex() of the bounds and their errors, the counts and SHA-256 of the q and samples arrays to
tests/golden/bounds_parent_bits.json (or argv[1]).  The committed fixture was written with the library of the commit before
the kernels were given shared bodies; rerun it only at a commit whose bits are meant to become the record."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import bounds_bits_case as bb  # noqa: E402
from options_model_amd import _ffi  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bounds_parent_bits.json")
ctx = _ffi.default_context(0)
rec = {c["name"]: bb.run(ctx, c) for c in bb.cases()}
for name, r in rec.items():
    print(name, float.fromhex(r["lower"]), float.fromhex(r["upper"]), r["n_exercised_lower"], r["inner_path_steps"])
with open(out, "w") as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write("\n")

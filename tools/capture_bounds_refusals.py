"""Record what the eight bounds facades of options_model_amd.api refuse, and in which order, for
tests/test_bounds_facade_refusals_cpu.py.

Runs the table of tests/helpers/bounds_refusal_cases.py -- per facade every invalid keyword set alone and every unordered
pair of them, on device 10^6 -- with the package of the tree it is started in and writes the type and the full message of the
exception each call raises first (each distinct message once, the calls as indices into that list) to
tests/golden/bounds_facade_refusals.json (or argv[1]).  No GPU is needed.  The committed fixture was written by the commit
before the facades were put on shared argument checks (its "commit" entry, argv[2], names it); rerun it only at a commit whose
messages and order are meant to become the record."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from helpers import bounds_refusal_cases as rc  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bounds_facade_refusals.json")
rec = dict(commit=sys.argv[2] if len(sys.argv) > 2 else "", **rc.record())
for name, f in rec["facades"].items():
    reached = sum(rec["messages"][i] == rc.REACHED for i in f["first"])
    print(f"{name}: {len(f['sets'])} sets, {len(f['first'])} calls, {len(set(f['first']))} distinct outcomes, "
          f"{reached} reach the context")
text = json.dumps(rec, indent=1, sort_keys=True)
text = re.sub(r"\[\s+((?:\d+,\s+)*\d+)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text)  # indices: one line
with open(out, "w") as f:
    f.write(text + "\n")

"""examples/american_greeks.c: a plain C host prints the config-2 Greeks through the ABI, the numbers the Python binding
returns for the same call."""
import os
import re
import shutil
import subprocess

import pytest

from options_model_amd import _build, _ffi

pytestmark = pytest.mark.gpu


def test_c_host_example_prints_config2_greeks(tmp_path, ctx):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    lib = _build.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "american_greeks"
    subprocess.run(["gcc", "-O2", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "american_greeks.c"), "-o", str(exe), "-L", os.path.dirname(lib),
                    "-lomc", "-lm", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    out = subprocess.run([str(exe), "200000", "50"], check=True, capture_output=True, text=True, timeout=300).stdout
    ref = ctx.price_american_greeks(_ffi.make_params(semantics="two_pass", n_paths=200000, n_steps=50, seed=42))
    assert abs(float(re.search(r"price ([-0-9.]+)", out).group(1)) - ref["price"]) < 1e-6
    for k in ("delta", "gamma", "vega", "rho", "theta"):
        v = float(re.search(rf"^{k} ([-0-9.]+)", out, flags=re.M).group(1))
        assert abs(v - ref[k]) <= 1e-6 + 1e-6 * abs(ref[k]), (k, v, ref[k])
    assert "storage: antithetic-folded" in out and ref["folded"] == 1

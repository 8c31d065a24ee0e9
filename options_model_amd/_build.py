"""In-tree build of libomc.so (HIP kernels + C ABI) for gfx950 with hipcc.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting
options_model_amd/lib/libomc.so travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
LIB = os.path.join(LIBDIR, "libomc.so")
SOURCES = ["omc_paths.hip", "omc_lsm.hip", "omc_batch.hip", "omc_mlp.hip", "omc_mlp_batch.hip", "omc_mlp_apply.hip", "omc_nn_epoch.hip", "omc_contnet.hip", "omc_rows.hip", "omc_ols7.hip", "omc_greeks.hip", "omc_barrier.hip", "omc_dividend.hip", "omc_jump.hip", "omc_basket.hip", "omc_bounds.hip", "omc_basket_bounds.hip", "omc_runnerup_bounds.hip", "omc_asian_bounds.hip", "omc_heston_bounds.hip", "omc_heston_sv_bounds.hip", "omc_jump_bounds.hip", "omc_dividend_bounds.hip", "omc_dividend_greeks.hip", "omc_jump_greeks.hip", "omc_barrier_bounds.hip", "omc_basket_greeks.hip", "omc_chain.hip", "omc_chain_bounds.hip", "omc_chain_greeks.hip", "omc_comm.hip", "omc_p2p.hip",
           "omc_api.hip", "omc_api_price.hip", "omc_api_seq.hip", "omc_api_batch.hip", "omc_api_nn.hip",
           "omc_api_bounds.hip", "omc_api_chain.hip", "omc_api_dividend.hip", "omc_api_jump.hip", "omc_api_basket.hip",
           "omc_api_basket_bounds.hip", "omc_api_runnerup_bounds.hip", "omc_api_basket_greeks.hip",
           "omc_api_heston_bounds.hip", "omc_api_jump_bounds.hip", "omc_api_dividend_bounds.hip",
           "omc_api_barrier_bounds.hip", "omc_api_dividend_greeks.hip", "omc_api_chain_bounds.hip",
           "omc_api_jump_greeks.hip", "omc_api_chain_greeks.hip"]
HEADERS = ["omc_ctx.h", "omc_device.h", "omc_dispatch.h", "omc_crit.h", "omc_kernels.h", "omc_lsm_dev.h", "omc_paths_dev.h", "omc_contnet_dev.h", "omc_mlp_dev.h", "omc_mlp_quad_dev.h", "omc_batch.h", "omc_greeks.h", "omc_greeks_dev.h", "omc_chain_greeks.h", "omc_barrier.h", "omc_dividend.h", "omc_jump.h", "omc_jump_dev.h", "omc_jump_bounds.h", "omc_dividend_bounds.h", "omc_dividend_greeks.h", "omc_jump_greeks.h", "omc_barrier_bounds.h", "omc_basket.h", "omc_basket_dev.h", "omc_bounds.h", "omc_bounds_dev.h", "omc_bounds_law_dev.h", "omc_bounds_sched_dev.h", "omc_bounds_cv_dev.h", "omc_bounds_check_dev.h", "omc_bounds2_dev.h", "omc_basket_bounds.h", "omc_runnerup_bounds.h", "omc_asian_bounds.h", "omc_asian_dev.h", "omc_heston_bounds.h", "omc_heston_sv_bounds.h", "omc_basket_greeks.h", "omc_chain.h", "omc_chain_bounds.h", "omc_chain_bounds_dev.h", "omc_comm.h", "omc_p2p.h",
           os.path.join("..", "..", "include", "omc.h"), os.path.join("..", "..", "include", "omc_jump_bounds.h"),
           os.path.join("..", "..", "include", "omc_dividend_bounds.h"),
           os.path.join("..", "..", "include", "omc_barrier_bounds.h"),
           os.path.join("..", "..", "include", "omc_dividend_greeks.h"),
           os.path.join("..", "..", "include", "omc_chain_bounds.h"),
           os.path.join("..", "..", "include", "omc_jump_greeks.h"),
           os.path.join("..", "..", "include", "omc_chain_greeks.h")]
ARCH = "gfx950"
# The extra compiler flags the library was built with (OMC_HIPCC_FLAGS: experiment builds such as
# -DOMC_DIAG_BUILD) are recorded next to it: a library left behind by an experiment is
# stale for every process that does not ask for the same flags, so tests / bench / profiles can never
# silently run a non-default build.
FLAGS_STAMP = os.path.join(LIBDIR, "libomc.flags")


def _flags() -> str:
    return " ".join(os.environ.get("OMC_HIPCC_FLAGS", "").split())


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libomc.so cannot be built (ROCm toolchain required)")


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    try:
        built_with = open(FLAGS_STAMP).read().strip()
    except OSError:
        built_with = ""
    if built_with != _flags():
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    hipcc = _hipcc()
    objs = []
    procs = []
    for s in SOURCES:
        o = os.path.join(LIBDIR, s.replace(".hip", ".o"))
        cmd = [hipcc, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-c",
               "-Wall", "-Wno-unused-function", os.path.join(CSRC, s), "-o", o]
        cmd[1:1] = _flags().split()  # experiments (-D..., -save-temps)
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(o)
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    for f in os.listdir(LIBDIR):  # objects of sources that no longer exist must not travel to the GPU box
        if f.endswith(".o") and os.path.join(LIBDIR, f) not in objs:
            os.remove(os.path.join(LIBDIR, f))
    link = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
    if verbose:
        print(" ".join(link), flush=True)
    subprocess.check_call(link)
    with open(FLAGS_STAMP, "w") as f:
        f.write(_flags() + "\n")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose="-v" in sys.argv))

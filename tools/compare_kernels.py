#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees kernel by kernel.

A refactor of the host launch layer must leave every kernel's instruction stream alone.  This builds both trees with the
project's own build (options_model_amd/_build.py -v, so -O3 --offload-arch=gfx950 and the resource-usage remarks) and
OMC_HIPCC_FLAGS=-save-temps, each from a copy under --work so that neither tree's own library is replaced, and compares

  * per kernel, the lines of the device assembly between its entry label and .Lfunc_end, after comments are dropped and
    the function's number is taken out of its local labels (.LBB<n>_<m> -> .LBB_<m>);
  * the -Rpass-analysis=kernel-resource-usage numbers (SGPRs, VGPRs, AGPRs, scratch, LDS, occupancy, spills).

Kernels are matched by source file and demangled name.  Kernels of the parent that the branch no longer has are listed
(a change that removes instantiations names them in its description); a kernel that differs, or one only the branch
has, makes the exit status 1.

  git archive --prefix=parent/ HEAD^ | tar -x -C /tmp/cmp
  python tools/compare_kernels.py --parent /tmp/cmp/parent --branch . --work /tmp/cmp/work -o profiles/<name>_isa.txt

--no-build compares what an earlier run left under --work.
"""
from __future__ import annotations

import argparse
import os
import re
import shutil
import subprocess
import sys

DEVICE_ASM = "-hip-amdgcn-amd-amdhsa-gfx950.s"
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")
REMARK = re.compile(r"^remark: (\S+?):\d+:\d+:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]\s*$")


def build(tree: str, work: str) -> None:
    """Copy what the build reads into `work`, build there with -save-temps; temporaries land in work/temps."""
    if os.path.exists(work):
        shutil.rmtree(work)
    os.makedirs(os.path.join(work, "temps"))
    shutil.copytree(os.path.join(tree, "include"), os.path.join(work, "include"))
    pkg = os.path.join(work, "options_model_amd")
    os.makedirs(pkg)
    shutil.copytree(os.path.join(tree, "options_model_amd", "csrc"), os.path.join(pkg, "csrc"))
    shutil.copy(os.path.join(tree, "options_model_amd", "_build.py"), pkg)
    env = dict(os.environ, OMC_HIPCC_FLAGS="-save-temps")
    with open(os.path.join(work, "build.log"), "w") as log:
        subprocess.check_call([sys.executable, os.path.join(pkg, "_build.py"), "-v", "--force"],
                              cwd=os.path.join(work, "temps"), env=env, stdout=log, stderr=subprocess.STDOUT)


def demangle(names: list[str]) -> dict[str, str]:
    for tool in ("llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        exe = shutil.which(tool) or (tool if os.path.exists(tool) else None)
        if exe:
            out = subprocess.run([exe], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
            return dict(zip(names, out.splitlines()))
    return {n: n for n in names}


def kernels_of(asm_path: str) -> dict[str, list[str]]:
    """mangled kernel name -> normalised body lines"""
    lines = open(asm_path).read().splitlines()
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    start = {}
    for i, ln in enumerate(lines):
        head = ln.split(":", 1)[0]
        if ln and not ln[0].isspace() and head in names and head not in start:
            start[head] = i
    out = {}
    for name in names:
        body = []
        for ln in lines[start[name] + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = LOCAL_LABEL.sub(r".L\1_\2", ln.split(";", 1)[0]).strip()
            if ln:
                body.append(ln)
        else:
            raise RuntimeError(f"{asm_path}: no .Lfunc_end after {name}")
        out[name] = body
    return out


def resources_of(log_path: str) -> dict[str, dict[str, str]]:
    """mangled kernel name -> resource numbers.  The compilations run side by side and share the log, so the remarks are
    taken apart by the source file they name before they are read in order."""
    per_file: dict[str, list[str]] = {}
    for ln in open(log_path, errors="replace"):
        m = REMARK.match(ln)
        if m:
            per_file.setdefault(m.group(1), []).append(m.group(2))
    out: dict[str, dict[str, str]] = {}
    for texts in per_file.values():
        cur = None
        for t in texts:
            key, _, val = t.partition(":")
            if key.strip() == "Function Name":
                cur = out.setdefault(val.strip(), {})
            elif cur is not None:
                cur[key.strip()] = val.strip()
    return out


def collect(work: str):
    temps = os.path.join(work, "temps")
    res = resources_of(os.path.join(work, "build.log"))
    per_file = {}
    for f in sorted(os.listdir(temps)):
        if f.endswith(DEVICE_ASM):
            ks = kernels_of(os.path.join(temps, f))
            pretty = demangle(list(ks)) if ks else {}
            per_file[f[:-len(DEVICE_ASM)] + ".hip"] = {pretty[n]: (body, res.get(n)) for n, body in ks.items()}
    return per_file


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="source tree of the parent commit (an unpacked git archive)")
    ap.add_argument("--branch", default=".", help="source tree of the change")
    ap.add_argument("--work", required=True, help="scratch directory for the two builds")
    ap.add_argument("--no-build", action="store_true")
    ap.add_argument("-o", "--output", default="-")
    a = ap.parse_args()

    sides = {"parent": a.parent, "branch": a.branch}
    if not a.no_build:
        for side, tree in sides.items():
            build(tree, os.path.join(a.work, side))
    parent, branch = (collect(os.path.join(a.work, side)) for side in sides)

    body, only_parent, only_branch = [], [], []
    n_cmp = n_same = n_diff = n_res = n_nores = 0
    for src in sorted(set(parent) | set(branch)):
        kp, kb = parent.get(src, {}), branch.get(src, {})
        body.append(f"== {src}: {len(kp)} kernels in the parent, {len(kb)} in the branch")
        for name in sorted(set(kp) | set(kb)):
            if name not in kb:
                only_parent.append((src, name))
                body.append(f"  ONLY IN THE PARENT  {name}")
            elif name not in kp:
                only_branch.append((src, name))
                body.append(f"  ONLY IN THE BRANCH  {name}")
            else:
                (ap_, rp), (ab, rb) = kp[name], kb[name]
                n_cmp += 1
                if rp is None or rb is None:
                    n_nores += 1
                if ap_ == ab and rp == rb:
                    n_same += 1
                    body.append(f"  identical ({len(ab)} lines)  {name}")
                else:
                    n_diff += ap_ != ab
                    n_res += rp != rb
                    what = "DIFFERENT" if ap_ != ab else "RESOURCES DIFFER"
                    body.append(f"  {what} ({len(ap_)} -> {len(ab)} lines; {rp} -> {rb})  {name}")

    head = [f"kernels compared: {n_cmp}; identical: {n_same}; instruction streams that differ: {n_diff}",
            f"kernels whose resource usage differs: {n_res}" + (f" (no resource remark found for {n_nores})" if n_nores else ""),
            f"kernels only in the parent: {len(only_parent)}; kernels only in the branch: {len(only_branch)}"]
    for title, lst in (("only in the parent", only_parent), ("only in the branch", only_branch)):
        if lst:
            head.append("")
            head.append(f"{title}:")
            head += [f"  {src}  {name}" for src, name in lst]
    text = "\n".join(head + [""] + body) + "\n"
    if a.output == "-":
        sys.stdout.write(text)
    else:
        with open(a.output, "w") as f:
            f.write(text)
        print("\n".join(head))
    return 1 if (n_diff or n_res or only_branch or n_nores) else 0


if __name__ == "__main__":
    sys.exit(main())

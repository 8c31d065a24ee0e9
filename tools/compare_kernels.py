#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees kernel by kernel.

A refactor of the host launch layer must leave every kernel's instruction stream alone.  This builds both trees with the
project's own build (options_model_amd/_build.py -v, so -O3 --offload-arch=gfx950 and the resource-usage remarks) and
OMC_HIPCC_FLAGS=-save-temps, each from a copy under --work so that neither tree's own library is replaced, and compares

  * per kernel, the lines of the device assembly between its entry label and .Lfunc_end, after comments are dropped and
    the function's number is taken out of its local labels (.LBB<n>_<m> -> .LBB_<m>) and the kernel's own mangled name
    is replaced by a placeholder; the directive that returns to the code section behind the kernel descriptor is dropped
    (.text for a plain function, a comdat section of its own for a template instantiation: where the linker puts the
    code, not what the code is);
  * the resource numbers (SGPRs, VGPRs, AGPRs, scratch, LDS, occupancy, code length): the "; Kernel info:" block the
    compiler writes behind each kernel in the assembly.  (The -Rpass-analysis=kernel-resource-usage remarks of the build
    log carry the same numbers, but the compilations run side by side and share the log: lines of one process are lost to,
    or land among, another's, and a kernel is then read with its neighbour's numbers.  The log is kept for the reader.)

Kernels are matched by source file and demangled name.  A change that renames kernels gives --renames a table of them,
one "parent demangled name => branch demangled name" per line (# starts a comment): a kernel of the parent that the table
names is compared with its partner in the branch's build of the same source file.  Kernels of the parent that the branch
no longer has are listed (a change that removes instantiations names them in its description); a kernel that differs, one
only the branch has, or an entry of the table whose kernel is missing on its side, makes the exit status 1.

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


def kernels_of(asm_path: str) -> dict[str, tuple[list[str], dict[str, str]]]:
    """mangled kernel name -> (normalised body lines, the numbers of its "; Kernel info:" block)"""
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
        for at, ln in enumerate(lines[start[name] + 1:], start[name] + 1):
            if ln.startswith(".Lfunc_end"):
                break
            ln = LOCAL_LABEL.sub(r".L\1_\2", ln.split(";", 1)[0]).replace(name, "<this kernel>").strip()
            if ln and ln != ".text" and not ln.startswith(".section\t.text."):
                body.append(ln)
        else:
            raise RuntimeError(f"{asm_path}: no .Lfunc_end after {name}")
        info = {}
        at = lines.index("; Kernel info:", at)
        while at + 1 < len(lines) and lines[at + 1].startswith(";"):
            at += 1
            key, _, val = lines[at][1:].partition(":" if ":" in lines[at] else "=")
            info[key.strip()] = val.strip()
        out[name] = (body, info)
    return out


def collect(work: str):
    temps = os.path.join(work, "temps")
    per_file = {}
    for f in sorted(os.listdir(temps)):
        if f.endswith(DEVICE_ASM):
            ks = kernels_of(os.path.join(temps, f))
            pretty = demangle(list(ks)) if ks else {}
            per_file[f[:-len(DEVICE_ASM)] + ".hip"] = {pretty[n]: ks[n] for n in ks}
    return per_file


def renames_of(path: str | None) -> dict[str, str]:
    table = {}
    for ln in open(path) if path else ():
        ln = ln.split("#", 1)[0].strip()
        if ln:
            old, _, new = ln.partition(" => ")
            table[old.strip()] = new.strip()
    return table


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True, help="source tree of the parent commit (an unpacked git archive)")
    ap.add_argument("--branch", default=".", help="source tree of the change")
    ap.add_argument("--work", required=True, help="scratch directory for the two builds")
    ap.add_argument("--no-build", action="store_true")
    ap.add_argument("--renames", help="table of renamed kernels: parent demangled name => branch demangled name")
    ap.add_argument("-o", "--output", default="-")
    a = ap.parse_args()

    sides = {"parent": a.parent, "branch": a.branch}
    if not a.no_build:
        for side, tree in sides.items():
            build(tree, os.path.join(a.work, side))
    parent, branch = (collect(os.path.join(a.work, side)) for side in sides)

    renames = renames_of(a.renames)
    unused = set(renames)
    body, only_parent, only_branch, renamed = [], [], [], []
    n_cmp = n_same = n_diff = n_res = n_nores = 0
    for src in sorted(set(parent) | set(branch)):
        kp, kb = parent.get(src, {}), branch.get(src, {})
        for old in [n for n in kp if n in renames and n not in kb]:  # the parent's kernel under its new name
            unused.discard(old)
            if renames[old] in kb and renames[old] not in kp:
                kp[renames[old]] = kp.pop(old)
                renamed.append((src, old, renames[old]))
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
                if not rp or not rb:
                    n_nores += 1
                if ap_ == ab and rp == rb:
                    n_same += 1
                    body.append(f"  identical ({len(ab)} lines)  {name}")
                else:
                    n_diff += ap_ != ab
                    n_res += rp != rb
                    what = "DIFFERENT" if ap_ != ab else "RESOURCES DIFFER"
                    body.append(f"  {what} ({len(ap_)} -> {len(ab)} lines; {rp} -> {rb})  {name}")

    gone = {(src, old) for src, old, _ in renamed}
    body += ["", f"== renamed ({len(renamed)} kernels, compared above under their new names)"]
    body += [f"  {src}  {old}  =>  {new}" for src, old, new in renamed]
    unpaired = sorted(unused) + [f"{src}  {n}" for src, n in only_parent if n in renames and (src, n) not in gone]
    head = [f"kernels compared: {n_cmp} ({len(renamed)} of them through the rename table); identical: {n_same}; "
            f"instruction streams that differ: {n_diff}",
            f"kernels whose resource usage differs: {n_res}" + (f" (no kernel info found for {n_nores})" if n_nores else ""),
            f"kernels only in the parent: {len(only_parent)}; kernels only in the branch: {len(only_branch)}"]
    if unpaired:
        head += ["", "entries of the rename table without a pair:"] + [f"  {u}" for u in unpaired]
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
    return 1 if (n_diff or n_res or only_branch or n_nores or unpaired) else 0


if __name__ == "__main__":
    sys.exit(main())

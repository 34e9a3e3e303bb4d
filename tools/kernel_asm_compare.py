"""Per-kernel comparison of the gfx950 assembly of csrc/vss_step.hip between two source trees.

    python tools/kernel_asm_compare.py PARENT_TREE [THIS_TREE] > profiles/<name>_asm_compare.log

Each tree's vss_step.hip is compiled with the Makefile's STEP_FLAGS to device assembly (-S
--offload-device-only); comments and directives are dropped and the local label numbers
(.LBB<function>_<block>) normalised, so two kernels compare equal exactly when their instruction
sequences are the same.  Resource usage comes from -Rpass-analysis=kernel-resource-usage, and each
kernel gets one more line on its prologue (the loads and waits in front of its first physics
instruction, see `prologue`).  A cross-compile: no GPU is needed.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -ffp-contract=off".split()
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_asm(tree: str):
    """{demangled kernel: [instructions]}, {demangled kernel: resource line} of the tree's vss_step.hip."""
    src = os.path.join(tree, "rsoccer-isaac-cleanrl_amd", "csrc", "vss_step.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "step.s")
        run = subprocess.run([HIPCC, *FLAGS, "-S", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage",
                              "-o", out, src], capture_output=True, text=True, check=True)
        with open(out) as f:
            lines = f.read().splitlines()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M))
    body, cur = {}, None
    for ln in lines:
        ln = ln.split(";")[0].rstrip()
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in kernels:
            cur = m.group(1)
            body[cur] = []
            continue
        if cur is None or not ln.strip():
            continue
        if re.match(r"^\s*\.(section|text|rodata|amdhsa_kernel|amdgpu_metadata)", ln) or ln.startswith(".Lfunc_end"):
            cur = None if ln.startswith(".Lfunc_end") or ".section" in ln else cur
            continue
        if ln.lstrip().startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", ln):
                body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
            continue
        body[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", ln.strip()))
    names = subprocess.run(["c++filt", *body], capture_output=True, text=True, check=True).stdout.split("\n")
    demangled = dict(zip(body, names))
    res, name = {}, None
    for ln in run.stderr.splitlines():
        m = re.search(r"remark: .*?(Function Name|VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            res[name] = {}
        elif name is not None:
            res[name][m.group(1).split(" ")[0]] = m.group(2)
    fmt = {demangled[k]: "VGPRs {VGPRs} AGPRs {AGPRs} SGPRs {SGPRs} scratch {ScratchSize} B/lane, LDS {LDS} B, "
                         "occupancy {Occupancy} waves/SIMD".format(**res[k]) for k in body if k in res}
    return {demangled[k]: v for k, v in body.items()}, fmt


def prologue(ins):
    """The loads and waits in front of a kernel's first physics instruction, in one line.

    The prologue runs from the kernel's entry to its first v_permlane32_swap (the physics, or the OU draws
    of the wrapped modes), or, where a kernel has none, to its first store to global memory.  Reported:
    the `s_waitcnt vmcnt` in it, the global loads issued before the first of those waits and behind it
    (position of the last load and of the first wait, as instruction indices), the backward branches
    (a load -> wait -> ds_write loop is one) and the s_load batches (runs of s_load with no other
    instruction but s_ ALU between them) with the lgkmcnt waits.
    """
    end = next((i for i, s in enumerate(ins) if s.startswith("v_permlane32_swap")), None)
    if end is None:
        end = next((i for i, s in enumerate(ins) if re.match(r"(global|buffer)_store", s)), len(ins))
    pro = ins[:end]
    waits = [i for i, s in enumerate(pro) if s.startswith("s_waitcnt") and "vmcnt" in s]
    loads = [i for i, s in enumerate(pro) if s.startswith("global_load")]
    labels = {s[:-1]: i for i, s in enumerate(pro) if s.endswith(":")}
    back = sum(1 for i, s in enumerate(pro)
               if s.startswith("s_cbranch") and labels.get(s.split()[-1], len(pro)) < i)
    first = waits[0] if waits else len(pro)
    sloads = [i for i, s in enumerate(pro) if s.startswith("s_load")]
    batches = sum(1 for k, i in enumerate(sloads)
                  if k == 0 or any(s.startswith("s_waitcnt") for s in pro[sloads[k - 1]:i]))
    return (f"prologue {len(pro)} instructions: {len(waits)} vmcnt waits, {len(loads)} global loads, "
            f"{sum(1 for i in loads if i < first)} before the first wait (at {first}), "
            f"{sum(1 for i in loads if i > first)} behind it (last load at {loads[-1] if loads else '-'}), "
            f"{back} backward branches, s_load in {batches} batches")


def main(argv):
    parent, tree = argv[1], argv[2] if len(argv) > 2 else REPO
    pa, pr = device_asm(parent)
    ta, tr = device_asm(tree)
    for asm, res in ((pa, pr), (ta, tr)):
        for k in res:
            res[k] += "\n             " + prologue(asm[k])
    new = [k for k in ta if k not in pa]
    gone = [k for k in pa if k not in ta]
    print("gfx950 assembly of vss_step.hip per kernel symbol, parent commit against this tree.")
    print(f"hipcc {' '.join(FLAGS)} -S --offload-device-only (the Makefile's STEP_FLAGS);")
    print("comments and directives dropped, local label numbers (.LBB<function>_) normalised; resource usage from")
    print("-Rpass-analysis=kernel-resource-usage.  "
          f"{len(pa)} symbols in the parent, {len(ta)} in this tree, {len(new)} new, {len(gone)} gone.\n")
    for k in ta:
        if k in new:
            print(f"new        {k}\n           {len(ta[k])} instructions; {tr.get(k, '?')}")
        elif pa[k] == ta[k]:
            print(f"identical  {k}\n           {len(ta[k])} instructions; {tr.get(k, '?')}")
        else:
            print(f"differs    {k}\n           parent {len(pa[k])} instructions; {pr.get(k, '?')}\n"
                  f"           tree   {len(ta[k])} instructions; {tr.get(k, '?')}")
    for k in gone:
        print(f"gone       {k}")
    return 1 if gone or any(k not in new and pa[k] != ta[k] for k in ta) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

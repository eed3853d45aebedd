#!/usr/bin/env python3
"""VALU instructions of tci_cohort_kernel<2,1,SS> per basic block, from the gfx950 disassembly, and
their sum along a path of blocks (the fast path of an evaluating wave, the path of a rejected row).

Every v_* instruction of a block is put into one class:
  fp64    FP64 arithmetic, compares, conversions and rcp/floor/ceil/ldexp (4 issue cycles per wave64)
  move    v_mov_b32 / v_mov_b64 / v_mov_b32_dpp / v_readlane / v_readfirstlane
  select  v_cndmask
  b32     every other 32-bit one (address arithmetic, integer compares)
The compiler's blocks follow the phases of eval_wave closely enough to name them: --phases gives
name=block,block,... groups; blocks of the path that no group names are listed as `other`.

usage: python scripts/lk_valu_table.py [-DTCI_LK_VALU=n] --path B1,B2,... [--reject-path ...]
       [--phases name=B1+B2,...] [--pmc pmc_summary.json --evals E --rejected R] [--asm FILE]
Blocks are named as in the assembly: `LBB24_0` for a label, `bb.12` for a fall-through block.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNEL = "_ZN3tci12_GLOBAL__N_117tci_cohort_kernelILi2ELi1ELi0EEE"


def disassembly(defs):
    from transcriptioncycleinference_amd.build import FILE_FLAGS

    src = os.path.join(ROOT, "transcriptioncycleinference_amd", "csrc", "tci_kernels.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-mllvm",
                        "-amdgpu-mfma-vgpr-form", "-fPIC", f"-I{ROOT}/include", f"-I{os.path.dirname(src)}",
                        "--cuda-device-only", "-S", src, "-o", out, "-Wno-pass-failed", *defs, *FILE_FLAGS[src]],
                       check=True, capture_output=True)
        return open(out).read()


def blocks(text):
    """block name -> list of instructions of the kernel, in order."""
    on, cur, out = False, "entry", {"entry": []}
    for line in text.splitlines():
        if line.startswith(KERNEL) and ":" in line.split(";")[0]:
            on = True
            continue
        if not on:
            continue
        if line.startswith("\t.section"):
            break
        m = re.match(r"^\.(LBB\d+_\d+):", line) or re.match(r"^; %(bb\.\d+):", line)
        if m:
            cur = m.group(1)
            out.setdefault(cur, [])
            continue
        ins = line.split(";")[0].strip()
        if ins and not ins.startswith("."):
            out[cur].append(ins)
    return out


def klass(ins):
    op = ins.split()[0]
    if not op.startswith("v_"):
        return None
    if op.startswith(("v_mov_b", "v_readlane", "v_readfirstlane", "v_writelane")):
        return "move"
    if op.startswith("v_cndmask"):
        return "select"
    if "_f64" in op or op.endswith(("_i64_e32", "_i64_e64", "_u64_e32", "_u64_e64")):
        return "fp64"
    return "b32"


def count(bl, names):
    c = {"fp64": 0, "b32": 0, "move": 0, "select": 0}
    for n in names:
        for ins in bl[n]:
            k = klass(ins)
            if k:
                c[k] += 1
    c["valu"] = sum(c.values())
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", required=True)
    ap.add_argument("--reject-path", default="")
    ap.add_argument("--phases", default="")
    ap.add_argument("--pmc")
    ap.add_argument("--evals", type=float, default=0)
    ap.add_argument("--rejected", type=float, default=0)
    ap.add_argument("--asm")
    a, defs = ap.parse_known_args()
    bl = blocks(open(a.asm).read() if a.asm else disassembly(defs))
    path = a.path.split(",")
    missing = [b for b in path if b not in bl]
    if missing:
        sys.exit(f"no such block: {missing}; blocks: {list(bl)}")
    out = {"kernel": "tci_cohort_kernel<2,1,SS>", "defines": defs, "static_valu": count(bl, list(bl))["valu"],
           "path": path, "per_block": {b: count(bl, [b]) for b in path}, "path_total": count(bl, path)}
    named = set()
    if a.phases:
        out["phases"] = {}
        for spec in a.phases.split(","):
            name, bs = spec.split("=")
            bs = bs.split("+")
            named.update(bs)
            out["phases"][name] = count(bl, bs)
        out["phases"]["other"] = count(bl, [b for b in path if b not in named])
    if a.reject_path:
        out["reject_path_total"] = count(bl, a.reject_path.split(","))
    if a.pmc:
        insts = json.load(open(a.pmc))["counters_mean_per_launch"]["SQ_INSTS_VALU"]
        rej = out.get("reject_path_total", {"valu": 0})["valu"] * a.rejected
        out["check"] = {"SQ_INSTS_VALU_per_launch": insts, "evaluating_waves": a.evals, "rejected_waves": a.rejected,
                        "measured_valu_per_evaluation": (insts - rej) / a.evals,
                        "table_valu_per_evaluation": out["path_total"]["valu"]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

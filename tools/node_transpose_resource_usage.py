#!/usr/bin/env python3
"""Register, scratch and LDS use of every kernel that walks the 4-wide nodes, parent commit against this tree, without a GPU.

Both trees are compiled for gfx950 with the Makefile's flags; the figures are `.vgpr_count`, `.sgpr_count`,
`.private_segment_fixed_size` (scratch) and `.group_segment_fixed_size` (static LDS) of the code-object metadata that
-save-temps leaves in the device assembly.  The budget of the transposed-node change: no kernel that had 0
scratch and <= 168 VGPRs (three waves per SIMD) may lose either.  Writes profiles/node_transpose_resource_usage.txt:

    python tools/node_transpose_resource_usage.py [--parent REV]     (REV: HEAD for uncommitted changes, else HEAD~1)

Other changes reuse it: --out FILE and --title TEXT name the listing and what "after" is, --same REGEX names kernels whose four
figures must not move at all (figures, not code: the frame gate's listing, profiles/frame_gate_resource_usage.txt, was made with
    --out profiles/frame_gate_resource_usage.txt --title "frame gate" \
        --same 'k_trace_primary(_compact)?<.*true(, (true|false))?>$|k_trace_primary<\\w+, \\w+, \\w+, true'
-- the VIEWS instantiations of the frame kernels, with or without RAYCAM, and the HINT instantiation, none of which is gated).
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("cg-raytracer_amd", "csrc")
UNITS = ["trace_kernels.hip", "variant_kernels.hip", "shade_kernels.hip", "surface_kernels.hip", "closest_kernels.hip", "crossing_kernels.hip",
         "prim_kernels.hip"]
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero", "-save-temps"]
VGPR_BUDGET = 168  # three waves per SIMD


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"^void |\([^()]*(\([^()]*\)[^()]*)*\)$", "", o.replace("(anonymous namespace)", "{anonymous}")) for o in out]


def usage(csrc_dir: str, unit: str, work: str) -> dict:
    """{kernel name: (VGPRs, SGPRs, scratch, LDS)} of one translation unit, from the metadata of its device assembly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(work, exist_ok=True)
    r = subprocess.run([hipcc, *FLAGS, "-I", csrc_dir, "-c", os.path.join(csrc_dir, unit), "-o", "unit.o"], cwd=work, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    asm = glob.glob(os.path.join(work, "*gfx950*.s"))
    if len(asm) != 1:
        sys.exit(f"expected one gfx950 assembly file in {work}, found {asm}")
    text = open(asm[0]).read()
    meta = text[text.index("amdhsa.kernels:"):]
    res = {}
    names, vals = [], []
    for block in re.split(r"\n  - ", meta)[1:]:
        get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block)  # noqa: E731
        if not get("vgpr_count"):
            continue
        names.append(get("name").group(1))
        vals.append((int(get("vgpr_count").group(1)), int(get("sgpr_count").group(1)), int(get("private_segment_fixed_size").group(1)),
                     int(get("group_segment_fixed_size").group(1))))
    for n, v in zip(demangle(names), vals):
        res[n] = v
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="revision to compare with (default: HEAD when the kernel sources differ from it, else HEAD~1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "node_transpose_resource_usage.txt"))
    ap.add_argument("--title", default="transposed 4-wide nodes", help="what the 'after' column is")
    ap.add_argument("--same", default=None, metavar="REGEX", help="kernels (demangled names) whose four figures must be unchanged")
    a = ap.parse_args()
    if a.parent is None:
        dirty = subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", CSRC, "include"]).returncode != 0
        a.parent = "HEAD" if dirty else "HEAD~1"
    before, after = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        for u in UNITS:
            before.update(usage(os.path.join(tmp, CSRC), u, os.path.join(tmp, "a_" + u)))
            after.update(usage(os.path.join(ROOT, CSRC), u, os.path.join(tmp, "b_" + u)))
    fmt = lambda v: " ".join(f"{x:>4}" for x in v)  # noqa: E731
    lines = ["hipcc --offload-arch=gfx950 -O3 (the Makefile's flags), code-object metadata of every kernel of " + ", ".join(UNITS) + ":",
             f"before (parent commit) and after ({a.title}).  Columns: .vgpr_count .sgpr_count .private_segment_fixed_size (scratch,",
             f"B/lane) .group_segment_fixed_size (static LDS, B/block).  Budget: a kernel with 0 scratch and <= {VGPR_BUDGET} VGPRs keeps both."
             + (f"  Kernels matching /{a.same}/ keep all four figures (the figures, not the code: kernel argument offsets may move)." if a.same else ""), ""]
    broken = 0
    for k in sorted(set(before) | set(after)):
        if k not in before or k not in after:
            lines.append(f"{fmt(before.get(k, ())):>20} -> {fmt(after.get(k, ())):<20} {'ONE SIDE ONLY':<14} {k}")
            broken += 1
            continue
        b, n = before[k], after[k]
        bad = (b[2] == 0 and n[2] > 0) or (b[0] <= VGPR_BUDGET and n[0] > VGPR_BUDGET) or (n[2] > b[2])
        bad = bad or bool(a.same and re.search(a.same, k) and b != n)
        broken += bad
        moved = " ".join(f"{f} {y - x:+d}" for f, x, y in zip(("vgpr", "sgpr", "scratch", "lds"), b, n) if x != y)
        note = "OVER BUDGET" if bad else (moved or "same")
        lines.append(f"{fmt(b):>20} -> {fmt(n):<20} {note:<14} {k}")
    lines += ["", f"kernels: {len(after)}; kernels that gained scratch, crossed {VGPR_BUDGET} VGPRs or moved although listed under --same: {broken}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if broken else 0


if __name__ == "__main__":
    sys.exit(main())

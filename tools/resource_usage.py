#!/usr/bin/env python3
"""Register, scratch and LDS use of every kernel of the library, a parent revision against this tree, without a GPU.

Every .hip file of both trees is compiled for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage.  Existing
kernels that changed or disappeared are reported and make the exit status 1; new kernels are listed, and may be held to limits:

    python tools/resource_usage.py --title "winding numbers" --out profiles/winding_resource_usage.txt --max-vgprs 128 --no-scratch --no-lds
    [--parent REV] [--jobs N]     (REV: HEAD for uncommitted changes, else HEAD~1)

ROOT, CSRC, demangle, usage, tree_usage and parent_tree are what the other *_resource_usage.py tools import.
"""
from __future__ import annotations

import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("cg-raytracer_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero", "-Rpass-analysis=kernel-resource-usage"]
FIELDS = [("VGPRs", r"VGPRs: (\d+)"), ("SGPRs", r"SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    # (a kernel of an anonymous namespace keeps its name: the argument list is cut at the first parenthesis AFTER that qualifier)
    return [re.sub(r"^void |\(.*$", "", o.replace("(anonymous namespace)::", "")) for o in out]


def usage(csrc_dir: str, src: str, obj: str) -> dict:
    """{kernel name: (VGPRs, SGPRs, scratch, LDS, waves)} of one translation unit."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, *FLAGS, "-c", src, "-o", obj], cwd=csrc_dir, capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = demangle([b.split()[0] for b in blocks])
    res = {}
    for name, b in zip(names, blocks):
        res[name] = tuple(int(re.search(pat, b).group(1)) for _, pat in FIELDS)
    return res


def tree_usage(csrc_dir: str, tmp: str, tag: str, jobs: int) -> dict:
    """{"file.hip: kernel name": usage} of every .hip file of csrc_dir."""
    srcs = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc_dir, "*.hip")))
    with ThreadPoolExecutor(jobs) as pool:
        parts = pool.map(lambda s: (s, usage(csrc_dir, s, os.path.join(tmp, f"{tag}_{s}.o"))), srcs)
        return {f"{s}: {k}": v for s, u in parts for k, v in u.items()}


def parent_tree(rev: str | None, tmp: str) -> tuple[str, str]:
    """The library's sources at `rev` unpacked under tmp: (rev, their csrc directory).  rev None: HEAD when the tree differs from it, else HEAD~1."""
    if rev is None:
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", CSRC, "include"], capture_output=True, text=True).stdout.strip()
        rev = "HEAD" if dirty else "HEAD~1"
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], capture_output=True, check=True).stdout
    subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
    return rev, os.path.join(tmp, CSRC)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="revision to compare with (default: HEAD when the sources differ from it, else HEAD~1)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resource_usage.txt"))
    ap.add_argument("--title", default="this tree", help="what the tree adds, for the report's heading")
    ap.add_argument("--max-vgprs", type=int, default=None, help="limit for new kernels")
    ap.add_argument("--no-scratch", action="store_true", help="new kernels may use no scratch")
    ap.add_argument("--no-lds", action="store_true", help="new kernels may use no LDS")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        rev, parent_csrc = parent_tree(a.parent, tmp)
        before = tree_usage(parent_csrc, tmp, "a", a.jobs)
        after = tree_usage(os.path.join(ROOT, CSRC), tmp, "b", a.jobs)
    fmt = lambda v: " ".join(str(x) for x in v)  # noqa: E731
    lines = ["hipcc --offload-arch=gfx950 -O3 (the Makefile's flags) -Rpass-analysis=kernel-resource-usage on every .hip file, before (parent",
             f"{rev}) and after ({a.title}).  Columns: VGPRs SGPRs scratch(B/lane) LDS(B/block) waves/SIMD.", ""]
    changed = [k for k in sorted(before) if after.get(k) != before[k]]
    lines.append(f"== existing kernels: {len(before)}, of which changed or gone: {len(changed)}")
    lines += [f"{fmt(before[k]):>18} -> {fmt(after[k]) if k in after else '(gone)':<18} CHANGED   {k}" for k in changed]
    new = sorted(set(after) - set(before))
    limits = [w for w, on in ((f"more than {a.max_vgprs} VGPRs", a.max_vgprs is not None), ("scratch", a.no_scratch), ("LDS", a.no_lds)) if on]
    lines += ["", f"== new kernels: {len(new)}"]
    over = 0
    for k in new:
        v = after[k]
        bad = (a.max_vgprs is not None and v[0] > a.max_vgprs) or (a.no_scratch and v[2] > 0) or (a.no_lds and v[3] > 0)
        over += bad
        lines.append(f"{fmt(v):>18}  {k}{'   OVER THE LIMIT' if bad else ''}")
    lines += ["", f"existing kernels changed or gone: {len(changed)}; new kernels: {len(new)}"
              + (f"; new kernels with {' or '.join(limits)}: {over}" if limits else "")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if changed or over else 0


if __name__ == "__main__":
    sys.exit(main())

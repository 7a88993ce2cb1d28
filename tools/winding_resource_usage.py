#!/usr/bin/env python3
"""Register, scratch and LDS use of every kernel of the library, parent commit against this tree, without a GPU: the winding-number
kernel adds a translation unit and must leave every existing kernel as it was.  Its instantiations are to use no
scratch, no LDS (the walk is stackless) and at most 128 VGPRs.

Every .hip file of both trees is compiled for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage.  Writes
profiles/winding_resource_usage.txt:

    python tools/winding_resource_usage.py [--parent REV] [--jobs N]     (REV: HEAD for uncommitted changes, else HEAD~1)
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from raycams_resource_usage import CSRC, ROOT  # noqa: E402
from sdf_resource_usage import tree_usage  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="revision to compare with (default: HEAD when the sources differ from it, else HEAD~1)")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_resource_usage.txt"))
    a = ap.parse_args()
    if a.parent is None:
        dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", CSRC, "include"], capture_output=True, text=True).stdout.strip()
        a.parent = "HEAD" if dirty else "HEAD~1"
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        before = tree_usage(os.path.join(tmp, CSRC), tmp, "a", a.jobs)
        after = tree_usage(os.path.join(ROOT, CSRC), tmp, "b", a.jobs)
    fmt = lambda v: " ".join(str(x) for x in v)  # noqa: E731
    lines = ["hipcc --offload-arch=gfx950 -O3 (the Makefile's flags) -Rpass-analysis=kernel-resource-usage on every .hip file, before (parent",
             "commit) and after (winding numbers).  Columns: VGPRs SGPRs scratch(B/lane) LDS(B/block) waves/SIMD.", ""]
    changed = [k for k in sorted(before) if after.get(k) != before[k]]
    lines.append(f"== existing kernels: {len(before)}, of which changed or gone: {len(changed)}")
    lines += [f"{fmt(before[k]):>18} -> {fmt(after[k]) if k in after else '(gone)':<18} CHANGED   {k}" for k in changed]
    lines += ["", "== new kernels: k_winding<GRID (0 list, 1 brick), COUNT, BRUTE>"]
    over = 0  # new instantiations with scratch, LDS or more than 128 VGPRs
    for k in sorted(set(after) - set(before)):
        bad = after[k][2] > 0 or after[k][3] > 0 or after[k][0] > 128
        over += bad
        lines.append(f"{fmt(after[k]):>18}  {k}{'   OVER THE TARGET' if bad else ''}")
    lines += ["", f"existing kernels changed: {len(changed)}; new kernels with scratch, LDS or more than 128 VGPRs: {over}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if changed or over else 0


if __name__ == "__main__":
    sys.exit(main())

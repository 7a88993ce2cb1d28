#!/usr/bin/env python3
"""Register, scratch and LDS use of every kernel of trace_kernels.hip, parent commit against this tree, without a GPU.

Both trees are compiled for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage.  Template arguments that
a tree's kernels gained at the end and that are false are dropped from the names, so that an existing instantiation keeps its name.
Writes profiles/raycams_resource_usage.txt:

    python tools/raycams_resource_usage.py [--parent REV]     (REV: HEAD for uncommitted changes, else HEAD~1)
"""
from __future__ import annotations

import argparse
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from resource_usage import CSRC, ROOT, parent_tree, usage  # noqa: E402


def trim(name: str) -> str:
    """Drop trailing `false` template arguments (arguments a later tree added are false for the kernels that existed)."""
    m = re.match(r"(.*)<(.*)>$", name)
    if not m:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    while args and args[-1] == "false":
        args.pop()
    return f"{m.group(1)}<{', '.join(args)}>" if args else m.group(1)


def twin(name: str):
    """The Trackball VIEWS twin of a RAYCAM instantiation: the same arguments without the trailing `true`."""
    m = re.match(r"(cgrt::k_trace_primary(?:_compact)?)<(.*), true>$", name)
    if not m:
        return None
    nargs = 6 if m.group(1).endswith("primary") else 5
    return trim(f"{m.group(1)}<{m.group(2)}>") if len(m.group(2).split(",")) == nargs - 1 else None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="revision to compare with (default: HEAD when the kernel sources differ from it, else HEAD~1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycams_resource_usage.txt"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        before = {trim(k): v for k, v in usage(parent_tree(a.parent, tmp)[1], "trace_kernels.hip", os.path.join(tmp, "a.o")).items()}
        after = {trim(k): v for k, v in usage(os.path.join(ROOT, CSRC), "trace_kernels.hip", os.path.join(tmp, "b.o")).items()}
    fmt = lambda v: " ".join(str(x) for x in v)  # noqa: E731
    lines = ["hipcc --offload-arch=gfx950 -O3 (the Makefile's flags) -Rpass-analysis=kernel-resource-usage on trace_kernels.hip, before (parent",
             "commit) and after (ray cameras).  Columns: VGPRs SGPRs scratch(B/lane) LDS(B/block) waves/SIMD.  Trailing `false` template",
             "arguments are dropped from the names: an existing instantiation keeps its name, the new trailing RAYCAM argument is false for it.", "",
             "== existing instantiations (before -> after)"]
    changed = 0
    for k in sorted(before):
        if k not in after:
            lines.append(f"{fmt(before[k]):>18} -> {'(gone)':<18} CHANGED   {k}")
            changed += 1
            continue
        same = before[k] == after[k]
        changed += not same
        lines.append(f"{fmt(before[k]):>18} -> {fmt(after[k]):<18} {'same' if same else 'CHANGED':<9} {k}")
    lines += ["", "== new instantiations (Trackball VIEWS twin -> new)"]
    worse = 0
    for k in sorted(set(after) - set(before)):
        t = twin(k)
        if t and t in after:
            bad = after[k][2] > after[t][2]
            worse += bad
            note = "scratch LARGER" if bad else ("more VGPRs" if after[k][0] > after[t][0] else "fits")
            lines.append(f"{fmt(after[t]):>18} -> {fmt(after[k]):<18} {note:<14} {k}   (twin {t})")
        else:
            lines.append(f"{'':>18}    {fmt(after[k]):<18} {'new':<9} {k}")
    lines += ["", f"existing instantiations changed: {changed}; new instantiations with more scratch than their twin: {worse}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 1 if changed or worse else 0


if __name__ == "__main__":
    sys.exit(main())

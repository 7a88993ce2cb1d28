"""Resource usage of the gfx950 kernels before and after the light-set kernels.

Compiles trace_kernels.hip and shade_kernels.hip of two source trees with -Rpass-analysis=kernel-resource-usage and writes one table:
every kernel of the old tree with its VGPRs, AGPRs, SGPRs, scratch and LDS on both sides (matched by name: no existing kernel was renamed),
then the new kernels.

    python tools/light_sets_resource_usage.py OLD_CSRC NEW_CSRC > profiles/light_sets_resource_usage.txt
"""
import re
import sys

from enqueue_resource_usage import FIELDS, demangle, report


def main(old_dir, new_dir):
    rows, changed = [], 0
    for src in ("trace_kernels.hip", "shade_kernels.hip"):
        old, new = report(old_dir, src), report(new_dir, src)
        dm_old, dm_new = demangle(list(old)), demangle(list(new))
        for k, dm in sorted(dm_old.items(), key=lambda kv: kv[1]):
            a, b = old[k], new.get(k, {})
            same = a == b
            changed += 0 if same else 1
            rows.append((src, "existing", dm, a, b, "same" if same else "CHANGED"))
        for k, dm in sorted(dm_new.items(), key=lambda kv: kv[1]):
            if k not in old:
                rows.append((src, "new", dm, {}, new[k], "scratch 0" if new[k].get("ScratchSize [bytes/lane]") == "0" else "SCRATCH"))
    print("# kernel resource usage, gfx950 (-Rpass-analysis=kernel-resource-usage): before -> after the light-set kernels")
    print("# columns: VGPRs AGPRs SGPRs scratch[B/lane] LDS[B/block]")
    fmt = lambda d: " ".join(d.get(f, "-") for f in FIELDS)  # noqa: E731
    for src, kind, dm, a, b, verdict in rows:
        dm = re.sub(r"\(.*", "", dm)
        print(f"{src:18s} {kind:8s} {verdict:9s} {fmt(a):>22s} -> {fmt(b):22s} {dm}")
    print(f"# existing instantiations changed: {changed}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

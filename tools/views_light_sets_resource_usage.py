"""Resource usage of the gfx950 kernels before and after the multi-view light-set kernels.

Compiles trace_kernels.hip and shade_kernels.hip of two source trees with -Rpass-analysis=kernel-resource-usage and writes one table:
every kernel of the old tree with its VGPRs, AGPRs, SGPRs, scratch and LDS on both sides (matched by name: no existing kernel was renamed),
then the new kernels.  The last lines compare the scratch of the new count-driven soft-shadow form (k_soft_shadow_sets_strided) with
k_soft_shadow_strided's, instantiation by instantiation.  Exit status 1 when an existing instantiation changed, a new shading kernel
uses scratch, or a new strided soft-shadow form spills more than its k_soft_shadow_strided<ANYHIT, FAST, true> counterpart.

    python tools/views_light_sets_resource_usage.py OLD_CSRC NEW_CSRC > profiles/views_light_sets_resource_usage.txt
"""
import re
import sys

from enqueue_resource_usage import FIELDS, demangle, report

SCRATCH = "ScratchSize [bytes/lane]"


def main(old_dir, new_dir):
    rows, changed, bad = [], 0, 0
    strided = {}  # "ANYHIT, FAST" -> (k_soft_shadow_strided<ANYHIT, FAST, true> scratch, k_soft_shadow_sets_strided<ANYHIT, FAST> scratch)
    for src in ("trace_kernels.hip", "shade_kernels.hip"):
        old, new = report(old_dir, src), report(new_dir, src)
        dm_old, dm_new = demangle(list(old)), demangle(list(new))
        for k, dm in sorted(dm_old.items(), key=lambda kv: kv[1]):
            a, b = old[k], new.get(k, {})
            same = a == b
            changed += 0 if same else 1
            rows.append((src, "existing", dm, a, b, "same" if same else "CHANGED"))
        for k, dm in sorted(dm_new.items(), key=lambda kv: kv[1]):
            m = re.search(r"k_soft_shadow_strided<(\w+, \w+), true>", dm)
            if m:
                strided.setdefault(m.group(1), [None, None])[0] = int(new[k].get(SCRATCH, "0"))
            if k in old:
                continue
            m = re.search(r"k_soft_shadow_sets_strided<(\w+, \w+)>", dm)
            if m:
                strided.setdefault(m.group(1), [None, None])[1] = int(new[k].get(SCRATCH, "0"))
            no_scratch = new[k].get(SCRATCH) == "0"
            if src == "shade_kernels.hip" and not no_scratch:
                bad += 1
            rows.append((src, "new", dm, {}, new[k], "scratch 0" if no_scratch else "SCRATCH"))
    print("# kernel resource usage, gfx950 (-Rpass-analysis=kernel-resource-usage): before -> after the multi-view light-set kernels")
    print("# columns: VGPRs AGPRs SGPRs scratch[B/lane] LDS[B/block]")
    fmt = lambda d: " ".join(d.get(f, "-") for f in FIELDS)  # noqa: E731
    for src, kind, dm, a, b, verdict in rows:
        dm = re.sub(r"\(.*", "", dm)
        print(f"{src:18s} {kind:8s} {verdict:9s} {fmt(a):>22s} -> {fmt(b):22s} {dm}")
    print(f"# existing instantiations changed: {changed}")
    print(f"# new shading kernels with scratch: {bad}")
    for key, (base, sets) in sorted(strided.items()):
        worse = base is None or sets is None or sets > base
        bad += 1 if worse else 0
        print(f"# scratch [B/lane] <{key}>: k_soft_shadow_strided (VIEWS) {base} / k_soft_shadow_sets_strided {sets}: "
              f"{'WORSE' if worse else 'no worse'}")
    return 1 if changed or bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

"""Resource usage of the gfx950 kernels before and after the count-driven (STRIDED) forms of enqueued frames.

Compiles trace_kernels.hip and shade_kernels.hip of two source trees with -Rpass-analysis=kernel-resource-usage and writes one table:
every kernel of the old tree with its VGPRs, AGPRs, SGPRs, scratch and LDS on both sides, then the new kernels.  Kernels that gained a
defaulted `STRIDED = false` template argument are matched to their old names by dropping that argument.

    python tools/enqueue_resource_usage.py OLD_CSRC NEW_CSRC > profiles/enqueue_resource_usage.txt
"""
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["-std=c++17", "-O3", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
         "-fno-gpu-flush-denormals-to-zero", "--offload-arch=gfx950", "--offload-device-only", "-Rpass-analysis=kernel-resource-usage"]
FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]"]


def report(csrc, src):
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-c", os.path.join(csrc, src), "-o", os.path.join(d, "k.o")],
                           capture_output=True, text=True, check=True)
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+([^:]+): (\S+) \[", line)
        if m and name and m.group(1) in FIELDS:
            out[name][m.group(1)] = m.group(2)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def old_name(dm):
    """the name the kernel had before its `STRIDED = false` argument (k_trace_batch, k_trace_shadow, k_trace_pair)"""
    return re.sub(r"(k_trace_(?:batch|shadow|pair)<[^>]*?), false>", r"\1>", dm)


def main(old_dir, new_dir):
    rows, changed = [], 0
    for src in ("trace_kernels.hip", "shade_kernels.hip"):
        old, new = report(old_dir, src), report(new_dir, src)
        dm_old, dm_new = demangle(list(old)), demangle(list(new))
        by_old = {}
        for k, dm in dm_new.items():
            by_old[old_name(dm)] = k
        seen = set()
        for k, dm in sorted(dm_old.items(), key=lambda kv: kv[1]):
            nk = by_old.get(dm)
            a = old[k]
            b = new.get(nk, {}) if nk else {}
            same = a == b
            changed += 0 if same else 1
            seen.add(nk)
            rows.append((src, "existing", dm, a, b, "same" if same else "CHANGED"))
        for k, dm in sorted(dm_new.items(), key=lambda kv: kv[1]):
            if k not in seen:
                rows.append((src, "new", dm, {}, new[k], "scratch 0" if new[k].get("ScratchSize [bytes/lane]") == "0" else "SCRATCH"))
    print("# kernel resource usage, gfx950 (-Rpass-analysis=kernel-resource-usage): before -> after the STRIDED forms")
    print("# columns: VGPRs AGPRs SGPRs scratch[B/lane] LDS[B/block]")
    fmt = lambda d: " ".join(d.get(f, "-") for f in FIELDS)
    for src, kind, dm, a, b, verdict in rows:
        dm = re.sub(r"\(.*", "", dm)
        print(f"{src:18s} {kind:8s} {verdict:9s} {fmt(a):>22s} -> {fmt(b):22s} {dm}")
    print(f"# existing instantiations changed: {changed}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))

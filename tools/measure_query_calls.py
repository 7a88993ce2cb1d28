"""Host wall time of the query entries' calls: the `dodge` scene of tests/golden, n = 4 096 queries, each host-pointer form and its
*_tensor form (the call plus a synchronisation of its stream): a warm-up, then the median of --calls calls, in milliseconds.

  python tools/measure_query_calls.py                      one process, one JSON line {name: median ms}
  python tools/measure_query_calls.py --compare libcgrt_parent.so --runs 6 --out profiles/query_calls_bench.txt
      runs alternating processes (parent, tree, parent, ...) with CGRT_LIB_NAME naming the library each loads from
      cg-raytracer_amd/lib, and writes the table: each of the tree's medians is to lie inside the parent's own min..max.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 4096


def measure(calls: int, warmup: int) -> dict:
    import numpy as np
    import torch

    import __graft_entry__ as entry

    pkg = entry.load_package()
    sd = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz"))
    sc = pkg.Scene(sd, device=0)
    rng = np.random.default_rng(7)
    pos = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, :3]
    lo, hi = pos.min(0), pos.max(0)
    points = (pos[rng.integers(0, len(pos), N)] + rng.normal(0, 0.05 * float((hi - lo).max()), (N, 3))).astype(np.float32)
    rays = np.zeros((N, 7), np.float32)
    rays[:, 0:3] = points
    d = rng.standard_normal((N, 3))
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 6] = np.inf
    d_points, d_rays = torch.from_numpy(points).cuda(), torch.from_numpy(rays).cuda()
    entries = {
        "occluded": lambda: sc.occluded(rays),
        "closest_points": lambda: sc.closest_points(points),
        "first_crossings(k=4)": lambda: sc.first_crossings(rays, 4),
        "nearest_triangles(k=8)": lambda: sc.nearest_triangles(points, 8),
        "sdf": lambda: sc.sdf(points),
        "winding_numbers": lambda: sc.winding_numbers(points),
        "occluded_tensor": lambda: sc.occluded_tensor(d_rays),
        "closest_points_tensor": lambda: sc.closest_points_tensor(d_points),
        "first_crossings_tensor(k=4)": lambda: sc.first_crossings_tensor(d_rays, 4),
        "nearest_triangles_tensor(k=8)": lambda: sc.nearest_triangles_tensor(d_points, 8),
        "sdf_tensor": lambda: sc.sdf_tensor(d_points),
        "winding_numbers_tensor": lambda: sc.winding_numbers_tensor(d_points),
    }
    out = {}
    for name, call in entries.items():
        times = []
        for i in range(warmup + calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if i >= warmup:
                times.append((time.perf_counter() - t0) * 1e3)
        out[name] = statistics.median(times)
    sc.close()
    return out


def compare(parent_lib: str, runs: int, calls: int, warmup: int, out_path: str) -> int:
    got = {"parent": [], "tree": []}
    for _ in range(runs):
        for who, name in (("parent", parent_lib), ("tree", "libcgrt.so")):
            env = dict(os.environ, CGRT_LIB_NAME=name)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(calls), "--warmup", str(warmup)], env=env,
                               capture_output=True, text=True, timeout=600)
            if r.returncode:
                print(r.stdout[-2000:], r.stderr[-2000:])
                return 1
            got[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    lines = [f"{runs} alternating processes (parent, tree, parent, ...) in one session on one MI355X of tools/measure_query_calls.py:",
             f"scene dodge, n = {N} queries, per process a warm-up of {warmup} calls, then the median wall time of {calls} calls, in ms (a *_tensor",
             "form: the call and a synchronisation of its stream).  parent: the parent commit's library; tree: this tree's; both under this",
             "tree's Python wrapper.  Each of the tree's medians is to lie inside the parent's own min..max.", ""]
    outside = 0
    for name in got["parent"][0]:
        p, t = [g[name] for g in got["parent"]], [g[name] for g in got["tree"]]
        med = statistics.median(t)
        inside = min(p) <= med <= max(p)
        outside += not inside
        word = "inside the parent's range" if inside else ("OUTSIDE the parent's range, " + ("below it" if med < min(p) else "ABOVE it"))
        lines += [name, "  parent runs: " + " ".join(f"{x:.4g}" for x in p) + f"   min {min(p):.4g} median {statistics.median(p):.4g} max {max(p):.4g}",
                  "  tree runs:   " + " ".join(f"{x:.4g}" for x in t) + f"   median {med:.4g}  -> {word}"]
    lines += ["", f"medians outside the parent's range: {outside}"]
    text = "\n".join(lines) + "\n"
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--compare", metavar="LIB", help="the parent's library in cg-raytracer_amd/lib (as CGRT_LIB_NAME names it)")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare, a.runs, a.calls, a.warmup, a.out)
    print(json.dumps(measure(a.calls, a.warmup)))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Closest-point queries (Scene.closest_points_tensor): the tree search k_closest against the brute-force kernel
k_closest_brute, and the search's work counters.

Scenes: dodge (16 311 triangles, tests/golden) and the 800 K dragon stand-in.  Query lists of 4 096, 65 536 and 1 048 576 points of two
families (tests/closest_ref.py): on the surface, and uniform in the scene box grown by 25 %.

Routes:
  tree    closest_points_tensor on the current stream: device time between HIP events, every shape warmed first, median and quartiles
  brute   closest_points_brute (the library has no device form of the validation path): wall time of the host call, which carries the
          44 bytes per query of its transfers; only where queries x triangles <= 2^34, fewer repetitions
  work    debug_closest_work on the first 65 536 queries at most: node steps and triangles evaluated per query (a counting launch, not timed)

  python3 tools/measure_closest.py [--reps N] [--out FILE.json] [--only NAME]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402
import closest_ref as cr  # noqa: E402

COUNTS = (4096, 65536, 1 << 20)
BRUTE_CAP = 1 << 34  # queries x triangles


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": float(med), "q1_ms": float(q1), "q3_ms": float(q3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_closest.py needs a GPU: a time taken elsewhere says nothing")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    pkg = entry.load_package()
    results = {"reps": a.reps, "source_hash": pkg.source_hash(), "scenes": {}}
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        res = {"ntris": sd.ntris, "families": {}}
        for fam, make in (("surface", cr.surface_queries), ("uniform", cr.uniform_queries)):
            allq = make(sd, max(COUNTS), 7)
            res["families"][fam] = {}
            for n in COUNTS:
                q = allq[:n]
                d_q = torch.from_numpy(q.copy()).cuda()
                out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
                for _ in range(5):  # warm: the code object, torch's allocator, the caches
                    sc.closest_points_tensor(d_q, out=out)
                torch.cuda.synchronize()
                events = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    sc.closest_points_tensor(d_q, out=out)
                    e1.record()
                    events.append((e0, e1))
                torch.cuda.synchronize()
                r = {"tree": quartiles([e0.elapsed_time(e1) for e0, e1 in events])}
                r["tree"]["queries_per_s"] = n / (r["tree"]["median_ms"] * 1e-3)
                if n * sd.ntris <= BRUTE_CAP:
                    got = out.cpu().numpy().view(pkg.CLOSEST_DTYPE).reshape(-1)
                    want = sc.closest_points_brute(q)  # (warms the call lane's buffers as well)
                    r["brute_bytes_equal"] = bool(got.tobytes() == want.tobytes())
                    walls = []
                    for _ in range(5):
                        t0 = time.perf_counter()
                        sc.closest_points_brute(q)
                        walls.append((time.perf_counter() - t0) * 1e3)
                    r["brute"] = quartiles(walls)
                else:
                    r["brute"] = None  # beyond BRUTE_CAP
                m = min(n, 65536)
                nodes, tris = sc.debug_closest_work(q[:m])
                r["work"] = {"queries": m, "node_steps_per_query": nodes / m, "triangles_per_query": tris / m}
                res["families"][fam][str(n)] = r
                print(name, fam, n, json.dumps(r))
        results["scenes"][name] = res
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Neighbour queries (Scene.nearest_triangles_tensor, count_neighbors_tensor, list_neighbors_tensor) against
closest_points_tensor on the same points, and the tree search against the brute-force entry.

Scenes: dodge (16 311 triangles, tests/golden) and the 800 K dragon stand-in.  1 048 576 points on the surface (tests/closest_ref.py).

Steps (device time between HIP events on the current stream, every shape warmed first, median and quartiles of --reps runs; a step whose
first run takes longer than a second is repeated 5 times only, its "n" says so):
  closest  closest_points_tensor: the floor and the yardstick
  k1       nearest_triangles_tensor, k = 1, unbounded (the same answer in 8 bytes per query); its ratio to closest
  k8       nearest_triangles_tensor, k = 8, unbounded
  radius   count_neighbors_tensor at 0.02 of the scene's extent, then the list call alone with the offsets of those counts (the full
           CSR list; skipped, with the reason, where it would exceed --max-records)
  brute    4 096 queries: nearest_triangles (k = 8) and list_neighbors_brute (k = 8), wall time of the host calls (median of --reps), and that
           their bytes agree
  work     debug_neighbor_work on the first 65 536 queries: node steps and triangles evaluated per query for k = 1, k = 8 and the count
           search at that radius (counting launches, not timed)

  python3 tools/measure_neighbors.py [--scene dodge|dragon800k] [--steps closest,k1,...] [--reps N] [--out profiles/neighbors_measure.json]

A run adds its scenes and steps to what --out already holds, so that every scene (or step) can run as a process of its own.
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

N = 1 << 20
STEPS = ("closest", "k1", "k8", "radius", "brute", "work")


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": float(med), "q1_ms": float(q1), "q3_ms": float(q3), "n": len(v)}


def timed(call, reps):
    """Device time of call() between events: warm runs (3; 1 where it takes longer than a second), then `reps` (5 in that case)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize()
    if time.perf_counter() - t0 > 1.0:
        reps = 5
    else:
        for _ in range(2):
            call()
        torch.cuda.synchronize()
    events = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        events.append((e0, e1))
    torch.cuda.synchronize()
    return quartiles([e0.elapsed_time(e1) for e0, e1 in events])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--scene", choices=("dodge", "dragon800k"))
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--max-records", type=int, default=1 << 30, help="the full list is skipped beyond this many records (8 bytes each)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_neighbors.py needs a GPU: a time taken elsewhere says nothing")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    steps = a.steps.split(",")
    pkg = entry.load_package()
    results = {"scenes": {}}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            results = json.load(f)
    results.update({"reps": a.reps, "source_hash": pkg.source_hash(), "queries": N})
    for name in ("dodge", "dragon800k"):
        if a.scene and a.scene != name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        lo, hi = cr.scene_box(sd)
        r2 = float(np.float32(np.float32(0.02 * float((hi - lo).max())) ** 2))
        res = results["scenes"].setdefault(name, {})
        res.update({"ntris": sd.ntris, "radius2": r2})
        q = cr.surface_queries(sd, N, 7)
        d_q = torch.from_numpy(q.copy()).cuda()
        if "closest" in steps:
            out = torch.empty((N, 8), dtype=torch.float32, device="cuda")
            res["closest"] = timed(lambda: sc.closest_points_tensor(d_q, out=out), a.reps)
            print(name, "closest", json.dumps(res["closest"]), flush=True)
            del out
        for k in (1, 8):
            if f"k{k}" in steps:
                out = torch.empty((N, k, 2), dtype=torch.float32, device="cuda")
                r = timed(lambda: sc.nearest_triangles_tensor(d_q, k, out=out), a.reps)
                if "closest" in res:
                    r["ratio_to_closest"] = r["median_ms"] / res["closest"]["median_ms"]
                res[f"k{k}"] = r
                print(name, f"k{k}", json.dumps(r), flush=True)
                del out
        if "radius" in steps:
            counts = torch.empty((N,), dtype=torch.int32, device="cuda")
            r = {"count": timed(lambda: sc.count_neighbors_tensor(d_q, r2, out=counts), a.reps)}
            offsets = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
            offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
            m = int(offsets[-1].item())
            r.update({"records": m, "mean_neighbours": m / N, "max_neighbours": int(counts.max().item())})
            if m > a.max_records:
                r["list"] = f"skipped: {m} records exceed --max-records {a.max_records}"
            else:
                records = torch.empty((max(m, 1), 2), dtype=torch.float32, device="cuda")
                s = torch.cuda.current_stream().cuda_stream
                r["list"] = timed(lambda: sc.list_neighbors_device(d_q.data_ptr(), N, records.data_ptr(), m, d_offsets_ptr=offsets.data_ptr(),
                                                                   max_dist2=r2, stream=s), a.reps)
                del records
            res["radius"] = r
            print(name, "radius", json.dumps(r), flush=True)
        if "brute" in steps:
            m = 4096
            tree = sc.nearest_triangles(q[:m], 8)  # (warms the call lane's buffers as well)
            brute, _ = sc.list_neighbors_brute(q[:m], k=8)
            r = {"queries": m, "k": 8, "bytes_equal": bool(tree.tobytes() == brute.tobytes())}
            for key, call in (("tree", lambda: sc.nearest_triangles(q[:m], 8)), ("brute", lambda: sc.list_neighbors_brute(q[:m], k=8))):
                walls = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    call()
                    walls.append((time.perf_counter() - t0) * 1e3)
                r[key] = quartiles(walls)
            res["brute"] = r
            print(name, "brute", json.dumps(r), flush=True)
        if "work" in steps:
            m = 65536
            r = {"queries": m}
            for key, kw in (("k1", {"k": 1}), ("k8", {"k": 8}), ("count_at_radius", {"max_dist2": r2})):
                nodes, tris = sc.debug_neighbor_work(q[:m], **kw)
                r[key] = {"node_steps_per_query": nodes / m, "triangles_per_query": tris / m}
            nodes, tris = sc.debug_closest_work(q[:m])
            r["closest"] = {"node_steps_per_query": nodes / m, "triangles_per_query": tris / m}
            res["work"] = r
            print(name, "work", json.dumps(r), flush=True)
        sc.close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
            print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()

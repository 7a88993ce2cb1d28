"""Point-set neighbours (Scene.point_grid_tensor, PointGrid): what a build and a query cost, the grid against the
brute form, and against torch.cdist + topk.

Clouds: stratified surface samples (Scene.sample_surface_tensor, strata = n, seed 1) of dodge (tests/golden) and of the 800 K dragon
stand-in, and a uniform unit cube; m = n, the cloud queried against itself with skip_same_index.  The squared radius aims at 16
neighbours: 16 A / (pi n) on a surface of area A, (16 / (n 4 pi / 3))^(2/3) in the cube; the grid's cell is that radius.

  * n = 65 536 and 1 048 576: the build alone (into a preallocated workspace), count, the 8 nearest within the radius (no counts), the
    full list (count, torch cumsum, list: one read-back in between) and knn with k = 8.  Each figure is the host's clock around `inner`
    calls that end in a device synchronisation, divided by `inner`; medians and quartiles of --reps repetitions after three warm ones.
  * n = 65 536: the 8 nearest within the radius through the host entries, the grid form against the brute form (which has a host form
    only), alternating within each repetition; both upload the same points and the grid form builds its grid in the call.
    `grid_beats_brute` is reported as measured, whichever way it falls.
  * n = 65 536, where the n x n matrix fits in memory: torch.cdist followed by topk(9, largest=False) on the same device (9: the point
    itself comes first), for the record; its indices are compared with knn's where the distances are distinct.

No time is asserted.

  python3 tools/measure_point_neighbors.py [--reps N] [--out profiles/point_neighbors_measure.json] [--only NAME] [--sizes 65536,1048576]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402


def wall(reps, routes, inner=1):
    """routes: name -> call.  Medians and quartiles in ms per call on the host's clock around `inner` calls and a device synchronisation,
    the routes alternating within each repetition."""
    for _ in range(3):
        for call in routes.values():
            call()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                call()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3 / inner)
    out = {}
    for k, v in t.items():
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        out[k] = {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_neighbors_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--brute-n", type=int, default=65536)
    ap.add_argument("--dragon", type=int, default=800_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_point_neighbors.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    cube_scene = pkg.Scene(pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cube.npz")), device=0)
    rows = []
    for name in ("dodge", "dragon800k", "uniform_cube"):
        if a.only and a.only not in name:
            continue
        if name == "uniform_cube":
            sc, area, tris = cube_scene, None, 0
        else:
            sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
                  else pkg.scenes.make_dragon(a.dragon))
            sc, tris = pkg.Scene(sd, device=0), int(sd.ntris)
            area = sc.triangle_areas()[1]
        for n in (int(x) for x in a.sizes.split(",")):
            if area is None:
                pts = torch.from_numpy(np.random.default_rng(1).random((n, 3)).astype(np.float32)).cuda()
                r2 = float(np.float32((16.0 / (n * 4.0 * math.pi / 3.0)) ** (2.0 / 3.0)))
            else:
                pts = sc.sample_surface_tensor(n, seed=1, strata=n)["point"].contiguous()
                r2 = float(np.float32(16.0 * area / (math.pi * n)))
            cell = math.sqrt(r2)
            torch.cuda.synchronize()
            row = {"cloud": name, "triangles": tris, "points": n, "radius2": r2, "cell": cell}
            nbytes = sc.point_grid_workspace(n)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            grid = sc.point_grid_tensor(pts, cell)
            counts = torch.empty((n,), dtype=torch.int32, device="cuda")
            near = torch.empty((n, 8, 2), dtype=torch.float32, device="cuda")
            kw = dict(max_dist2=r2, skip_same_index=True)
            inner = 10 if n <= 65536 else 3
            row.update(wall(a.reps, {
                "build": lambda: sc.point_grid_build_device(pts.data_ptr(), n, cell, ws.data_ptr(), nbytes,
                                                            stream=torch.cuda.current_stream().cuda_stream),
                "count": lambda: grid.count(pts, out=counts, **kw),
                "nearest8": lambda: grid.nearest(pts, 8, out=near, **kw),
            }, inner))
            row.update(wall(a.reps, {"full_list": lambda: grid.list(pts, **kw), "knn8": lambda: grid.knn(pts, 8, skip_same_index=True)}))
            c = counts.cpu().numpy()
            row.update({"grid_bytes": nbytes, "mean_neighbours": round(float(c.mean()), 2), "max_neighbours": int(c.max())})
            host = pts.cpu().numpy()
            work = sc.debug_point_neighbor_work(host, cell, host, **kw)
            row.update({"cells_per_query": round(work["cells"] / n, 2), "entries_read_per_query": round(work["entries"] / n, 2),
                        "foreign_entries_per_query": round(work["foreign"] / n, 2), "d2_per_query": round(work["d2_evals"] / n, 2),
                        "linear_queries": work["linear"], "buckets_used": work["buckets_used"]})
            if n == a.brute_n:
                got = {}
                few = max(3, a.reps // 4)
                t = wall(few, {"grid_host_form_nearest8": lambda: got.__setitem__("grid", sc.nearest_points(host, cell, host, 8, **kw)),
                               "brute_host_form_nearest8": lambda: got.__setitem__("brute", sc.list_point_neighbors_brute(host, host, k=8, **kw)[0])})
                row.update(t)
                row["same_bytes"] = bool(np.array_equal(got["grid"].view(np.uint32), got["brute"].view(np.uint32)))
                row["brute_over_grid"] = round(t["brute_host_form_nearest8"]["median_ms"] / t["grid_host_form_nearest8"]["median_ms"], 2)
                row["grid_beats_brute"] = t["grid_host_form_nearest8"]["median_ms"] < t["brute_host_form_nearest8"]["median_ms"]
                try:
                    res = {}
                    t = wall(few, {"torch_cdist_topk9": lambda: res.__setitem__("v", torch.topk(torch.cdist(pts, pts), 9, largest=False))})
                    row.update(t)
                    knn = grid.knn(pts, 8, skip_same_index=True)
                    idx = knn.view(torch.int32)[..., 1].cpu().numpy()
                    d = knn[..., 0].cpu().numpy()
                    distinct = (np.diff(d, axis=1) > 0).all(1)
                    tidx = res["v"].indices[:, 1:].cpu().numpy()
                    row["torch_same_indices_where_distinct"] = round(float((idx[distinct] == tidx[distinct]).all(1).mean()), 4)
                    del res
                except RuntimeError as e:  # (out of memory: the matrix did not fit)
                    row["torch_cdist_topk9"] = f"not measured: {str(e)[:80]}"
            rows.append(row)
            print(json.dumps(row), flush=True)
            del pts, ws, grid, counts, near
            torch.cuda.empty_cache()
        if sc is not cube_scene:
            sc.close()
    cube_scene.close()
    doc = {"device": torch.cuda.get_device_name(0), "sources": pkg.source_hash(), "reps": a.reps,
           "timing": "host clock around the calls and a device synchronisation, ms per call; routes of a group alternate within each repetition",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Winding numbers (Scene.winding_numbers_tensor, Scene.winding_grid_tensor): the tree form at beta = 2, 3 and 4
against the sum over every triangle (beta = inf on the device entry: the brute form's additions and bytes) and against the parity vote of
the signed-distance kernel (Scene.sdf_tensor(want="inside"), whose answer means something on closed meshes only) on the same points.

Scenes: dodge (tests/golden, open) and the 800 K dragon stand-in (closed).  Per scene
  list   1 048 576 points uniform in the scene box grown by 25 % (tests/closest_ref.py uniform_queries)
  grid   128^3 points over the same box: the tree form makes its own points (a wave = a 4 x 4 x 4 brick); the every-triangle route and
         the parity vote are given the grid's points as a ready tensor (sdf_grid_points, not timed)
The every-triangle route runs on every point of dodge; on the dragon it runs on 4 096 points only, as a row of its own.

Every route writes into preallocated tensors, is warmed first, and is timed between HIP events on the current stream; the routes of a row
ALTERNATE within each repetition, so that a drift of the machine hits them alike.  A row holds the median and quartiles of every route,
`spread` = (q3 - q1) / median of the beta = 2 route, the work counters per point (debug_winding_work on 65 536 points at most, a counting
launch, not timed), the largest |w(beta) - w(every triangle)| where that route ran, and how many verdicts differ from it.  No time is asserted.

  python3 tools/measure_winding.py [--reps N] [--out profiles/winding_measure.json] [--only NAME] [--n POINTS] [--side N]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402
import closest_ref as cr  # noqa: E402
from measure_sdf import timed  # noqa: E402

BETAS = (2.0, 3.0, 4.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "winding_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--dragon", type=int, default=800_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_winding.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    rows = []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(a.dragon))
        sc = pkg.Scene(sd, device=0)
        before = sc.device_bytes()
        lo, hi = cr.scene_box(sd)
        ext = np.maximum(hi - lo, 1e-3)
        origin, spacing, dims = lo - 0.25 * ext, 1.5 * ext / (a.side - 1), (a.side,) * 3
        shapes = {"list": cr.uniform_queries(sd, a.n, 7), "grid": pkg.sdf_grid_points(origin, spacing, dims)}
        if name != "dodge":
            shapes["list_4096"] = shapes["list"][:4096]
        for shape, pts in shapes.items():
            n = len(pts)
            d_pts = torch.from_numpy(pts).cuda()
            o_w = {b: torch.empty((n,), dtype=torch.float32, device="cuda") for b in BETAS + ("brute",)}
            o_i = torch.empty((n,), dtype=torch.bool, device="cuda")
            o_p = torch.empty((n,), dtype=torch.bool, device="cuda")
            with_brute = name == "dodge" or shape == "list_4096"
            routes = {}
            for b in BETAS:
                if shape == "grid":
                    routes[f"tree_beta{b:g}"] = lambda b=b: sc.winding_grid_tensor(origin, spacing, dims, beta=b, out=(o_w[b].view(dims[::-1]), o_i.view(dims[::-1])))
                else:
                    routes[f"tree_beta{b:g}"] = lambda b=b: sc.winding_numbers_tensor(d_pts, beta=b, out=(o_w[b], o_i))
            if with_brute:  # (the brute entry takes host pointers: timed here is the device form with no cluster far, beta = inf, which
                # performs the brute form's additions in its order, returns its bytes, and also reads every cluster)
                routes["every_triangle"] = lambda: sc.winding_numbers_tensor(d_pts, beta=float("inf"), out=(o_w["brute"], o_i))
            routes["sdf_inside"] = lambda: sc.sdf_tensor(d_pts, want="inside", out=o_p)
            t = timed(a.reps, routes)
            for call in routes.values():
                call()
            torch.cuda.synchronize()
            m = min(n, 65536)
            sub = pts[:: n // m][:m]
            work = {f"beta{b:g}": [round(x / m, 2) for x in sc.debug_winding_work(sub, beta=b)] for b in BETAS}
            t2 = t["tree_beta2"]
            row = {"scene": name, "triangles": int(sd.ntris), "shape": shape, "points": n, **t,
                   "spread": round((t2["q3_ms"] - t2["q1_ms"]) / t2["median_ms"], 4),
                   "work_per_point": {"columns": ["clusters tested", "dipoles taken", "triangles evaluated"], **work},
                   "parity_vote_differs_from_beta2_verdict": int(((o_w[2.0].abs() > 0.5) != o_p).sum().item())}
            if with_brute:
                wb = o_w["brute"].double()
                row["tree_beta2_faster_than_brute"] = t2["median_ms"] < t["every_triangle"]["median_ms"]
                row["speedup_beta2_over_brute"] = round(t["every_triangle"]["median_ms"] / t2["median_ms"], 3)
                row["max_abs_error_vs_brute"] = {f"beta{b:g}": float((o_w[b].double() - wb).abs().max().item()) for b in BETAS}
                row["verdicts_differing_from_brute"] = {f"beta{b:g}": int(((o_w[b].abs() > 0.5) != (wb.abs() > 0.5)).sum().item()) for b in BETAS}
            rows.append(row)
            print(json.dumps(row), flush=True)
        rows.append({"scene": name, "tree_device_bytes": int(sc.device_bytes() - before), "scene_device_bytes": int(before)})
        sc.close()
    doc = {"device": torch.cuda.get_device_name(0), "sources": pkg.source_hash(), "reps": a.reps,
           "timing": "device time between HIP events, ms; the routes of a row alternate within each repetition", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

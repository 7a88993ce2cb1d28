"""Iso-surfaces (Scene.isosurface_count_device, Scene.isosurface_device): extraction from SDF grids against the
call that made the values and against one torch pass over the grid.

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Per scene and per side (128, 256): the grid over the scene box grown by 25 %,
its values made by sdf_grid_tensor, the level 2 % of the largest extent off the surface.  Routes of a row:
  count   cgrt_isosurface_count_device alone
  list    cgrt_isosurface_device with exact capacities (it redoes the count inside its workspace)
  sdf     the sdf_grid_tensor call that made the values
  floor   (values < iso).sum(): a single torch pass over the grid
Outputs, counts and the workspace are preallocated; every route is warmed first and timed between HIP events on the current stream; the
routes ALTERNATE within each repetition, so that a drift of the machine hits them alike.  A row holds the median and quartiles of every
route, the spread (q3 - q1) / median of the list route, the counts, and each extraction route's ratio to the floor and to the SDF call.
No time is asserted.

  python3 tools/measure_isosurface.py [--reps N] [--out profiles/isosurface_measure.json] [--only NAME] [--sides 128,256]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--sides", default="128,256")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_isosurface.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    rows = []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        lo, hi = cr.scene_box(sd)
        ext = np.maximum(hi - lo, 1e-3)
        iso = float(np.float32(0.02 * ext.max()))
        for side in (int(x) for x in a.sides.split(",")):
            origin, spacing, dims = lo - 0.25 * ext, 1.5 * ext / (side - 1), (side,) * 3
            values = torch.empty(dims[::-1], dtype=torch.float32, device="cuda")
            sdf = lambda: sc.sdf_grid_tensor(origin, spacing, dims, want="sdf", out=values)  # noqa: E731
            sdf()
            nbytes = sc.isosurface_workspace(dims)
            ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
            counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            count = lambda: sc.isosurface_count_device(origin, spacing, dims, values.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,  # noqa: E731
                                                       iso=iso, stream=st)
            count()
            nv, nt = (int(x) for x in counts.cpu())
            verts = torch.empty((max(nv, 1), 3), dtype=torch.float32, device="cuda")
            tris = torch.empty((max(nt, 1), 3), dtype=torch.int32, device="cuda")
            lst = lambda: sc.isosurface_device(origin, spacing, dims, values.data_ptr(), verts.data_ptr(), nv, tris.data_ptr(), nt,  # noqa: E731
                                               counts.data_ptr(), ws.data_ptr(), nbytes, iso=iso, stream=st)
            t = timed(a.reps, {"count": count, "list": lst, "sdf": sdf, "floor": lambda: (values < iso).sum()})
            med = {k: v["median_ms"] for k, v in t.items()}
            row = {"scene": name, "triangles": int(sd.ntris), "side": side, "points": side**3, "iso": iso, "vertices": nv, "mesh_triangles": nt,
                   "workspace_bytes": nbytes, **t, "spread": round((t["list"]["q3_ms"] - t["list"]["q1_ms"]) / med["list"], 4),
                   "count_over_floor": round(med["count"] / med["floor"], 3), "list_over_floor": round(med["list"] / med["floor"], 3),
                   "count_over_sdf": round(med["count"] / med["sdf"], 4), "list_over_sdf": round(med["list"] / med["sdf"], 4)}
            rows.append(row)
            print(json.dumps(row), flush=True)
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

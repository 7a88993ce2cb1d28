"""Point-set frames (PointGrid.frames, PointGrid.knn_frames): what the fused search-and-solve kernel costs, next
to the search alone and to the composition it replaces.

Clouds: stratified surface samples (Scene.sample_surface_tensor, strata = n, seed 1) of dodge (tests/golden) and of the 800 K dragon
stand-in, and a uniform unit cube; n = 65 536 and 1 048 576, each cloud against itself with skip_same_index.  The squared radius aims
at 2 k neighbours: 2 k A / (pi n) on a surface of area A, (2 k / (n 4 pi / 3))^(2/3) in the cube; the grid's cell is that radius.  For k = 8
and k = 16, on one grid:

  * frames      PointGrid.frames within the radius (the neighbour records are written as well)
  * nearest     PointGrid.nearest alone on the same arguments: the search's share
  * knn_frames  the k nearest without a bound, by growing radii (it blocks)
  * torch       the composition the README used to show: PointGrid.knn, a gather, the centred products and torch.linalg.eigh (n 3 x 3
                problems), then the smallest eigenvector; its normals are compared with knn_frames' up to sign where the float64 gap
                (lambda1 - lambda0) / trace exceeds 1e-2

Each figure is the host's clock around `inner` calls that end in a device synchronisation, divided by `inner`; medians and quartiles of
--reps repetitions after three warm ones, the routes of a group alternating within each repetition.  No time is asserted and no ratio
promised: `frames_beats_torch` is reported as measured, whichever way it falls.

  python3 tools/measure_point_frames.py [--reps N] [--out profiles/point_frames_measure.json] [--only NAME] [--sizes 65536,1048576]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402
from measure_point_neighbors import wall  # noqa: E402


def torch_pca(grid, a, k):
    """The README's former composition: (normal (n, 3), eigenvalues (n, 3) of the covariance)."""
    idx = grid.knn(a, k, skip_same_index=True).view(torch.int32)[..., 1].long()
    nb = a[idx] - a[idx].mean(1, keepdim=True)
    w, v = torch.linalg.eigh(nb.transpose(1, 2) @ nb)
    return v[..., 0], w / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_frames_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--ks", default="8,16")
    ap.add_argument("--dragon", type=int, default=800_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_point_frames.py needs a GPU: a time taken elsewhere says nothing")
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
            else:
                pts = sc.sample_surface_tensor(n, seed=1, strata=n)["point"].contiguous()
            for k in (int(x) for x in a.ks.split(",")):
                if area is None:
                    r2 = float(np.float32((2.0 * k / (n * 4.0 * math.pi / 3.0)) ** (2.0 / 3.0)))
                else:
                    r2 = float(np.float32(2.0 * k * area / (math.pi * n)))
                cell = math.sqrt(r2)
                grid = sc.point_grid_tensor(pts, cell)
                torch.cuda.synchronize()
                row = {"cloud": name, "triangles": tris, "points": n, "k": k, "radius2": r2, "cell": cell}
                near = torch.empty((n, k, 2), dtype=torch.float32, device="cuda")
                kw = dict(max_dist2=r2, skip_same_index=True)
                inner = 10 if n <= 65536 else 3
                row.update(wall(a.reps, {"frames": lambda: grid.frames(pts, pts, k, **kw), "nearest": lambda: grid.nearest(pts, k, out=near, **kw)},
                                inner))
                few = a.reps if n <= 65536 else max(3, a.reps // 4)
                try:
                    row.update(wall(few, {"knn_frames": lambda: grid.knn_frames(pts, pts, k, skip_same_index=True),
                                          "torch_knn_gather_eigh": lambda: torch_pca(grid, pts, k)}))
                    row["frames_over_nearest"] = round(row["frames"]["median_ms"] / row["nearest"]["median_ms"], 3)
                    row["torch_over_knn_frames"] = round(row["torch_knn_gather_eigh"]["median_ms"] / row["knn_frames"]["median_ms"], 2)
                    row["frames_beats_torch"] = row["knn_frames"]["median_ms"] < row["torch_knn_gather_eigh"]["median_ms"]
                    fr = grid.knn_frames(pts, pts, k, skip_same_index=True)
                    tn, tw = torch_pca(grid, pts, k)
                    w = fr["eigenvalues"].double()
                    gap = (w[:, 1] - w[:, 0]) / w.sum(1).clamp_min(1e-300)
                    sel = gap > 1e-2
                    cosine = (fr["normal"][sel].double() * tn[sel].double()).sum(1).abs()
                    row["normals_compared"] = int(sel.sum().item())
                    row["normal_min_abs_cosine_against_torch"] = round(float(cosine.min().item()), 6)
                    row["eigenvalue_max_diff_over_trace_against_torch"] = float(((w - tw.double()).abs().max(1).values / w.sum(1).clamp_min(1e-300)).max().item())
                    del fr, tn, tw
                except RuntimeError as e:  # (out of memory in the composition)
                    row["torch_knn_gather_eigh"] = f"not measured: {str(e)[:80]}"
                used = grid.frames(pts, pts, k, **kw)["used"]
                row["mean_used_within_radius"] = round(float(used.float().mean().item()), 2)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del grid, near
                torch.cuda.empty_cache()
            del pts
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

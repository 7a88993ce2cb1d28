"""Ray cameras (Scene.render_raycams_tensor, cgrt_render_raycams_device) against the Trackball views and against the route a caller with
camera matrices had before them, in the same process, the order of the routes rotated from repeat to repeat:
  raycams     ONE render_raycams_tensor call for the B cameras, each fitted to its Trackball view with RayCamera.from_trackball;
  views       ONE render_views_tensor call for the B Trackball views (the frame kernels the ray cameras are instantiated next to);
  torch_list  the rays of all views generated in torch from the cameras' matrices (origin + M @ (x + 0.5, y + 0.5, 1), normalised, t =
              FLT_MAX; the pixel grid is made once up front, the generation itself is timed), then ONE shade_rays_tensor call over them.
Per route: median, minimum and maximum over the repeats of the host time of the whole batch up to a synchronize, and the median of the
library's device_ms.  The bar for `raycams` is the spread of `views` in the same run: its min-max range over the repeats.

  python3 tools/measure_raycams.py [--repeats N] [--out FILE.json] [--only NAME]
  python3 tools/measure_raycams.py --kernels NAME     (a few batches only: run under rocprofv3 --kernel-trace --stats)

Workloads (those of tools/measure_views.py): Cornell at depth 4 and the 800 K-triangle dragon stand-in at depth 2, B = 1, 4 and 16 views
of 256x256."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402
from measure_views import cameras, scene_of  # noqa: E402

WORKLOADS = [  # name, scene, depth, B, W, H
    ("cornell_b1_256", "cornell", 4, 1, 256, 256),
    ("cornell_b4_256", "cornell", 4, 4, 256, 256),
    ("cornell_b16_256", "cornell", 4, 16, 256, 256),
    ("dragon_b1_256", "dragon", 2, 1, 256, 256),
    ("dragon_b4_256", "dragon", 2, 4, 256, 256),
    ("dragon_b16_256", "dragon", 2, 16, 256, 256),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kernels", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    results = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "source_hash": pkg.source_hash(), "runs": []}
    for name, which, depth, B, W, H in WORKLOADS:
        if (a.only and name != a.only) or (a.kernels and name != a.kernels):
            continue
        sc = pkg.Scene(scene_of(pkg, which), device=0)
        cams = cameras(pkg, B, W, H)
        rcams = pkg.raycam_array([pkg.RayCamera.from_trackball(c, W, H) for c in cams])
        # the caller's matrices on the device: origin (B, 3) and M (B, 3, 3) with direction = M @ (x + 0.5, y + 0.5, 1)
        origin = torch.from_numpy(rcams[:, 0:3].copy()).to(dev)
        M = torch.from_numpy(np.stack([rcams[:, 12:15], rcams[:, 15:18], rcams[:, 9:12] - 0.5 * rcams[:, 12:15] - 0.5 * rcams[:, 15:18]], axis=2).copy()).to(dev)
        ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
        grid = torch.stack([xs + 0.5, ys + 0.5, torch.ones_like(xs)], dim=-1).reshape(-1, 3)  # (W*H, 3), made once
        tmax = torch.full((B, W * H, 1), float(np.finfo(np.float32).max), device=dev)
        out_ray = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        out_views = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        out_list = torch.empty((B * W * H, 3), dtype=torch.float32, device=dev)

        def raycams():
            return sc.render_raycams_tensor(rcams, W, H, out=out_ray, max_level=depth)[1]

        def views():
            return sc.render_views_tensor(cams, W, H, out=out_views, max_level=depth)[1]

        def torch_list():
            d = torch.matmul(grid[None], M.transpose(1, 2))  # (B, W*H, 3)
            d = d / torch.linalg.vector_norm(d, dim=-1, keepdim=True)
            rays = torch.cat([origin[:, None, :].expand(B, W * H, 3), d, tmax], dim=-1).reshape(-1, 7).contiguous()
            return sc.shade_rays_tensor(rays, out=out_list, max_level=depth)[1]

        routes = {"raycams": raycams, "views": views, "torch_list": torch_list}
        if a.kernels:
            for _ in range(5):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            print("kernels run done:", name)
            sc.close()
            continue
        for fn in routes.values():  # warm-up: workspaces grown
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        samples = {k: {"call_ms": [], "device_ms": []} for k in routes}
        keys = list(routes)
        for rep in range(a.repeats):
            for i in range(len(keys)):
                k = keys[(rep + i) % len(keys)]
                t0 = time.perf_counter()
                st = routes[k]()
                torch.cuda.synchronize()
                samples[k]["call_ms"].append((time.perf_counter() - t0) * 1e3)
                samples[k]["device_ms"].append(float(st["device_ms"]))
        r = {"workload": name, "scene": which, "depth": depth, "B": B, "W": W, "H": H}
        for k, v in samples.items():
            r[k] = {"call_ms": float(np.median(v["call_ms"])), "call_ms_min": float(np.min(v["call_ms"])), "call_ms_max": float(np.max(v["call_ms"])),
                    "device_ms": float(np.median(v["device_ms"])), "device_ms_min": float(np.min(v["device_ms"])),
                    "device_ms_max": float(np.max(v["device_ms"]))}
        for unit in ("call_ms", "device_ms"):
            spread = r["views"][unit + "_max"] - r["views"][unit + "_min"]
            r["views_spread_" + unit] = spread
            r["raycams_minus_views_" + unit] = r["raycams"][unit] - r["views"][unit]
            r["raycams_within_views_spread_" + unit] = bool(r["raycams"][unit] - r["views"][unit] <= spread)
        r["torch_list_over_raycams_call"] = r["torch_list"]["call_ms"] / r["raycams"]["call_ms"]
        # the fitted cameras draw the Trackball's frames up to the rays' last bits: how far apart the two batches are
        r["mean_abs_rgb_difference_raycams_views"] = float((out_ray - out_views).abs().mean().item())
        results["runs"].append(r)
        print(json.dumps(r), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

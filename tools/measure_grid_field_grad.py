"""The sampler's adjoint (Scene.sample_grid_grad_device) against the backward of
torch.nn.functional.grid_sample(align_corners=True) with respect to its input, on the same device.

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Per scene and per side (128, 256): the grid over the scene box grown by 25 %,
its values made by sdf_grid_tensor.  Two sets of 1 048 576 points:
  uniform   uniform in the grid's box
  surface   the hit points of march_grid_tensor from 1024 x 1024 camera rays (misses are replaced by hits drawn again, so that every
            point adds): concentrated on a surface, the contended case
Routes of a row, per set:
  value / gradient / both   sample_grid_grad_device with grad_value only, grad_gradient only, both, into a preallocated volume
  torch                     the backward of grid_sample's trilinear value with respect to the volume (torch.autograd.grad of a recorded
                            forward with retain_graph; the value alone: torch has no gradient output to differentiate)
Per route the added bytes per second, 4 x (non-zero contributions, counted by the numpy restatement on the same points) / median time,
beside the chip-wide rate of about 1.3 TB/s that float atomics reach when a wave's adds are contiguous (a microbenchmark figure).
Everything is preallocated; every route is warmed first and timed between HIP events on the current stream; the routes ALTERNATE within
each repetition, so that a drift of the machine hits them alike.  No time is asserted.

  python3 tools/measure_grid_field_grad.py [--reps N] [--out profiles/grid_field_grad_measure.json] [--only NAME] [--sides 128,256]
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
import grid_field_grad_ref as aref  # noqa: E402
from measure_grid_field import camera_rays  # noqa: E402
from measure_sdf import timed  # noqa: E402

ATOMIC_RATE_CONTIGUOUS = 1.3e12  # bytes of float adds per second, chip-wide, contiguous wave adds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_field_grad_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--sides", default="128,256")
    ap.add_argument("--rays-side", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_grid_field_grad.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    Fn = torch.nn.functional
    rows = []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        lo, hi = cr.scene_box(sd)
        ext = np.maximum(hi - lo, 1e-3)
        rays_h = camera_rays(lo, hi, a.rays_side)
        n = len(rays_h)
        rays = torch.from_numpy(rays_h).cuda()
        st = torch.cuda.current_stream().cuda_stream
        rng = np.random.default_rng(17)
        gv_h, gg_h = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        gv, gg = torch.from_numpy(gv_h).cuda(), torch.from_numpy(gg_h).cuda()
        for side in (int(x) for x in a.sides.split(",")):
            origin, spacing, dims = (lo - 0.25 * ext).astype(np.float32), (1.5 * ext / (side - 1)).astype(np.float32), (side,) * 3
            values = sc.sdf_grid_tensor(origin, spacing, dims, want="sdf")
            extent = float(ext.max())
            rec = sc.march_grid_tensor(values, origin, spacing, rays, iso=0.0, relax=1.0, min_step=1e-4 * extent, hit_eps=1e-4 * extent,
                                       max_steps=256, refine=8)
            hit = (rec["status"] == 1).cpu().numpy()
            if not hit.any():
                raise SystemExit(f"{name} {side}: no ray hit the level")
            t_h = rec["t"].cpu().numpy()
            surf = (rays_h[hit, 0:3] + t_h[hit, None] * rays_h[hit, 3:6]).astype(np.float32)
            surf = surf[np.random.default_rng(side).integers(0, len(surf), n)] if len(surf) < n else surf[:n]
            sets = {"uniform": (origin + np.random.default_rng(side).uniform(0, 1, size=(n, 3)) * (1.5 * ext)).astype(np.float32),
                    "surface": np.ascontiguousarray(surf)}
            o_t, s_t = torch.from_numpy(origin).cuda(), torch.from_numpy(spacing * (side - 1)).cuda()
            out = torch.zeros(dims[::-1], dtype=torch.float32, device="cuda")
            for set_name, pts_h in sets.items():
                pts = torch.from_numpy(pts_h).cuda()
                vol = torch.zeros_like(values)[None, None].requires_grad_(True)
                coords = ((pts - o_t) / s_t * 2 - 1)[None, None, None]
                sampled = Fn.grid_sample(vol, coords, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0, 0]

                def call(v, g):
                    return lambda: sc.sample_grid_grad_device(origin, spacing, dims, pts.data_ptr(), n, v.data_ptr() if v is not None else 0,
                                                              g.data_ptr() if g is not None else 0, out.data_ptr(), stream=st)

                routes = {"value": call(gv, None), "gradient": call(None, gg), "both": call(gv, gg),
                          "torch": lambda: torch.autograd.grad(sampled, vol, gv, retain_graph=True)}
                t = timed(a.reps, routes)
                adds, cells = {}, None
                for key, (v, g) in (("value", (gv_h, None)), ("gradient", (None, gg_h)), ("both", (gv_h, gg_h))):
                    inside, index, c = aref.contributions(origin, spacing, dims, pts_h, v, g)
                    adds[key] = int(np.count_nonzero(c))
                    if cells is None:
                        cells = int(len(np.unique(index[inside, 0])))
                row = {"scene": name, "triangles": int(sd.ntris), "side": side, "set": set_name, "n": n, "distinct_cells": cells,
                       "hit_fraction_of_rays": round(float(hit.mean()), 4), **t}
                for key in ("value", "gradient", "both"):
                    med = t[key]["median_ms"]
                    row[key + "_adds"] = adds[key]
                    row[key + "_added_TB_per_s"] = round(4.0 * adds[key] / (med * 1e-3) / 1e12, 4)
                    row[key + "_over_torch"] = round(med / t["torch"]["median_ms"], 3)
                    row["spread_" + key] = round((t[key]["q3_ms"] - t[key]["q1_ms"]) / med, 4)
                rows.append(row)
                print(json.dumps(row), flush=True)
        sc.close()
    doc = {"device": torch.cuda.get_device_name(0), "sources": pkg.source_hash(), "reps": a.reps,
           "timing": "device time between HIP events, ms; the routes of a row alternate within each repetition",
           "contiguous_atomic_rate_TB_per_s": ATOMIC_RATE_CONTIGUOUS / 1e12, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

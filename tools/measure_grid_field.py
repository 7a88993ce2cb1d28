"""Grid fields (Scene.sample_grid_device, Scene.march_grid_device): samples and marched rays on SDF grids against
torch.nn.functional.grid_sample on the same device, and against one closest-hit call on the mesh.

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Per scene and per side (128, 256): the grid over the scene box grown by 25 %,
its values made by sdf_grid_tensor.  Routes of a row:
  sample         1 M uniform points in the grid's box, value + gradient + inside
  grid_sample    torch's trilinear lookup of the same points (align_corners=True; the value alone, no gradient)
  march_relax1   1 M camera rays (1024 x 1024 pinhole looking at the box's centre), relax 1, min_step 1e-4 of the extent, 256 steps
  march_fixed    the same rays, relax 0, min_step = the spacing, refine 8, 1 024 steps
  torch_relax1 / torch_fixed   a torch loop of grid_sample steps over ALL rays, as many as the march's mean main-loop samples per ray that
                 entered the box (cgrt_debug_march_work): no hit test, no refinement, no early exit -- a floor for the same lookups
  closest_hit    one intersect call on the mesh with the same rays, for context
Everything is preallocated; every route is warmed first and timed between HIP events on the current stream; the routes ALTERNATE within
each repetition, so that a drift of the machine hits them alike.  No time is asserted.

  python3 tools/measure_grid_field.py [--reps N] [--out profiles/grid_field_measure.json] [--only NAME] [--sides 128,256]
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


def camera_rays(lo, hi, side=1024):
    """side x side pinhole rays from outside the box towards its centre, (n, 7) float32, unit directions."""
    c, ext = 0.5 * (lo + hi), float((hi - lo).max())
    eye = c + ext * np.asarray([1.1, 0.8, 1.6])
    fwd = (c - eye) / np.linalg.norm(c - eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    s = (np.arange(side) + 0.5) / side * 2 - 1
    half = np.tan(np.radians(20.0))
    d = fwd[None, None, :] + half * (s[None, :, None] * right[None, None, :] + s[::-1][:, None, None] * up[None, None, :])
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    r = np.zeros((side * side, 7), np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 6] = eye, d, np.finfo(np.float32).max
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_field_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--sides", default="128,256")
    ap.add_argument("--rays-side", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_grid_field.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    F = torch.nn.functional
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
        hits = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        mesh_hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        for side in (int(x) for x in a.sides.split(",")):
            origin, spacing, dims = (lo - 0.25 * ext).astype(np.float32), (1.5 * ext / (side - 1)).astype(np.float32), (side,) * 3
            values = sc.sdf_grid_tensor(origin, spacing, dims, want="sdf")
            rng = np.random.default_rng(side)
            pts_h = (origin + rng.uniform(0, 1, size=(n, 3)) * (1.5 * ext)).astype(np.float32)
            pts = torch.from_numpy(pts_h).cuda()
            val = torch.empty((n,), dtype=torch.float32, device="cuda")
            grad = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            ins = torch.empty((n,), dtype=torch.uint8, device="cuda")
            o_t, s_t = torch.from_numpy(origin).cuda(), torch.from_numpy(spacing * (side - 1)).cuda()
            vol = values[None, None]

            def lookup(p):  # torch's trilinear value at points (n, 3): x fastest, normalised to [-1, 1]
                return F.grid_sample(vol, ((p - o_t) / s_t * 2 - 1)[None, None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, 0, 0, 0]

            extent = float(ext.max())
            sets = {"relax1": dict(iso=0.0, relax=1.0, min_step=1e-4 * extent, hit_eps=1e-4 * extent, max_steps=256),
                    "fixed": dict(iso=0.0, relax=0.0, min_step=float(spacing.max()), hit_eps=1e-4 * extent, max_steps=1024, refine=8)}
            routes = {
                "sample": lambda: sc.sample_grid_device(origin, spacing, dims, values.data_ptr(), pts.data_ptr(), n, val.data_ptr(), grad.data_ptr(),
                                                        ins.data_ptr(), stream=st),
                "grid_sample": lambda: lookup(pts),
                "closest_hit": lambda: sc.intersect_device(rays.data_ptr(), n, mesh_hits.data_ptr(), stream=st),
            }
            info = {}
            for key, prm in sets.items():
                work = sc.debug_march_work(values.cpu().numpy(), origin, spacing, rays_h, **prm)
                sc.march_grid_device(origin, spacing, dims, values.data_ptr(), rays.data_ptr(), n, hits.data_ptr(), stream=st, **prm)
                status = hits.view(torch.int32)[:, 3]
                mean_steps = max(1, int(round(work[1] / max(work[0], 1))))
                info[key] = {"entered": work[0], "main_samples": work[1], "refine_samples": work[2], "mean_steps": mean_steps,
                             "hits": int((status == 1).sum()), "exhausted": int((status == 2).sum())}

                def torch_loop(prm=prm, steps=mean_steps):
                    t = torch.zeros((n,), dtype=torch.float32, device="cuda")
                    for _ in range(steps):
                        v = lookup(rays[:, 0:3] + t[:, None] * rays[:, 3:6])
                        t = t + torch.clamp(prm["relax"] * v, min=prm["min_step"])
                    return t

                routes["march_" + key] = lambda prm=prm: sc.march_grid_device(origin, spacing, dims, values.data_ptr(), rays.data_ptr(), n,
                                                                              hits.data_ptr(), stream=st, **prm)
                routes["torch_" + key] = torch_loop
            t = timed(a.reps, routes)
            med = {k: v["median_ms"] for k, v in t.items()}
            row = {"scene": name, "triangles": int(sd.ntris), "side": side, "points": side**3, "n": n, **t, "march": info,
                   "spread_sample": round((t["sample"]["q3_ms"] - t["sample"]["q1_ms"]) / med["sample"], 4),
                   "spread_march_relax1": round((t["march_relax1"]["q3_ms"] - t["march_relax1"]["q1_ms"]) / med["march_relax1"], 4),
                   "sample_over_grid_sample": round(med["sample"] / med["grid_sample"], 3),
                   "march_relax1_over_torch": round(med["march_relax1"] / med["torch_relax1"], 4),
                   "march_fixed_over_torch": round(med["march_fixed"] / med["torch_fixed"], 4),
                   "march_relax1_over_closest_hit": round(med["march_relax1"] / med["closest_hit"], 3)}
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

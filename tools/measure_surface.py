"""Surface attributes (Scene.surface_views_tensor, interpolate_hits_tensor) against what a caller would compose
from the barycentric output alone, and against a second trace for scale.  Device time between HIP events on the stream the work runs
on, every shape warmed first, the routes taken in turn (rotated from repetition to repetition); per route the median and the quartiles.

Workloads: (a) Cornell 1920 x 1080, frame form; (b) the 800 K dragon stand-in 1920 x 1080, frame form; (c) the same dragon frame's rays
as a list of 2 073 600 rays, list form.  Channels C = 3 and C = 32, a seeded random table.

Routes:
  bary          the surface call, barycentrics only
  attr          the surface call, the interpolated attribute only (the fused form)
  bary+attr     the surface call, both outputs
  bary+torch    the barycentrics from the surface call, then the attribute composed in torch: attr[tri[prim_id]] gathered three times,
                a weighted sum in the reference's order, zeros off the triangles
  trace         trace_views_device (frames) / intersect_device (list) of the same rays: what tracing again would cost

  python3 tools/measure_surface.py [--reps N] [--out FILE.json] [--only NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402

W, H = 1920, 1080
WORKLOADS = [("cornell_1080p_frame", "cornell", "frame"), ("dragon800k_1080p_frame", "dragon", "frame"), ("dragon800k_2m_list", "dragon", "list")]
CHANNELS = (3, 32)


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
        raise SystemExit("measure_surface.py needs a GPU: a time taken elsewhere says nothing")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    pkg = entry.load_package()
    results = {"reps": a.reps, "source_hash": pkg.source_hash(), "W": W, "H": H, "workloads": {}}
    scenes = {}
    for name, which, form in WORKLOADS:
        if a.only and a.only not in name:
            continue
        if which not in scenes:
            sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz")) if which == "cornell"
                  else pkg.scenes.make_dragon(800_000))
            scenes[which] = (sd, pkg.Scene(sd, device=0))
        sd, sc = scenes[which]
        cam = pkg.scenes.default_camera(W, H)
        n = W * H
        ntris, nverts = sd.ntris, len(sd.pos_nrm)
        tri = torch.from_numpy(np.asarray(sd.tri, np.int64).reshape(-1, 3)).cuda()
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        sc.trace_views_device(cam[None], W, H, hits.data_ptr())
        torch.cuda.synchronize()
        depth = hits[:, 0].view(torch.float32).reshape(1, H, W).contiguous()
        prim = hits[:, 1].reshape(1, H, W).contiguous()
        rays = torch.from_numpy(sc.generate_rays(cam, W, H).view(np.float32).reshape(-1, 7).copy()).cuda() if form == "list" else None
        hits2 = torch.empty_like(hits)
        on_tri = (prim.reshape(-1) >= 0) & (prim.reshape(-1) < ntris)
        rows = tri[prim.reshape(-1).clamp(0, max(ntris - 1, 0)).long()]
        res = {"triangle_hits": int(on_tri.sum().item()), "items": n, "channels": {}}
        for C in CHANNELS:
            attr = torch.from_numpy(np.random.default_rng(C).standard_normal((nverts, C)).astype(np.float32)).cuda()
            o_b = torch.empty((1, H, W, 3) if form == "frame" else (n, 3), dtype=torch.float32, device="cuda")
            o_a = torch.empty((1, H, W, C) if form == "frame" else (n, C), dtype=torch.float32, device="cuda")

            def surface(want_bary, want_attr):
                if form == "frame":
                    out = ({"bary": o_b} if want_bary else {}) | ({"attr": o_a} if want_attr else {})
                    sc.surface_views_tensor(cam, W, H, depth, prim, attr=attr if want_attr else None, want_bary=want_bary, out=out)
                else:
                    if want_bary:
                        sc.hit_barycentrics_tensor(rays, hits, out=o_b)
                    if want_attr:
                        sc.interpolate_hits_tensor(rays, hits, attr, out=o_a)

            def composed():
                surface(True, False)
                w = o_b.reshape(-1, 3)
                v = (w[:, 0:1] * attr[rows[:, 0]] + w[:, 1:2] * attr[rows[:, 1]]) + w[:, 2:3] * attr[rows[:, 2]]
                return torch.where(on_tri[:, None], v, torch.zeros((), dtype=torch.float32, device="cuda"))

            def trace():
                if form == "frame":
                    sc.trace_views_device(cam[None], W, H, hits2.data_ptr())
                else:
                    sc.intersect_device(rays.data_ptr(), n, hits2.data_ptr())

            routes = {"bary": lambda: surface(True, False), "attr": lambda: surface(False, True), "bary+attr": lambda: surface(True, True),
                      "bary+torch": composed, "trace": trace}
            order = list(routes)
            for _ in range(5):  # warm: code objects, the lookup table, torch's allocator
                for r in order:
                    routes[r]()
            torch.cuda.synchronize()
            surface(False, True)
            same = bool(torch.equal(composed().view(torch.int32), o_a.reshape(-1, C).view(torch.int32)))
            events = {r: [] for r in order}
            for i in range(a.reps):
                k = i % len(order)
                for r in order[k:] + order[:k]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    routes[r]()
                    e1.record()
                    events[r].append((e0, e1))
                torch.cuda.synchronize()
            res["channels"][str(C)] = {"routes": {r: quartiles([e0.elapsed_time(e1) for e0, e1 in v]) for r, v in events.items()},
                                       "torch_composition_bit_equal": same,
                                       "bytes_model": {"read_per_item": 8 if form == "frame" else 44, "read_per_triangle_hit": 16 + 48 + 12 * C,
                                                       "written_per_item": 4 * C}}
            print(name, "C", C, json.dumps(res["channels"][str(C)]["routes"]), "torch composition bit-equal:", same)
        results["workloads"][name] = res
    for _, sc in scenes.values():
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()

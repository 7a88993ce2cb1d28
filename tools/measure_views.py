"""Multi-view frames (Scene.render_views_tensor, cgrt_render_views_device) against the routes a caller has without them, in the same
process, the order of the routes rotated from repeat to repeat:
  views       ONE render_views_tensor call for the B cameras;
  exact       B render_tensor calls on one stream, prediction off (the exactly sized path every batch takes);
  predicted   B render_tensor calls, prediction on (the scene's previous frame of the shape sizes the next: the single frame's fastest path);
  list        ONE shade_rays_tensor call over all views' rays, each view's rays in 8x8-tile order, concatenated (the rays
              are generated once up front and not timed; the colours come back as a ray list, not in the frame formats).
Per route: median over the repeats of the host time of the whole batch up to a synchronize, and of the library's device_ms (summed over
the calls of a route).  The views' frames are checked bit for bit against the exact route's.

  python3 tools/measure_views.py [--repeats N] [--out FILE.json] [--only NAME]
  python3 tools/measure_views.py --kernels NAME     (a few batches only: run under rocprofv3 --kernel-trace --stats)

Workloads: Cornell at depth 4, B = 1, 4, 16, 64 views of 256x256 and 16 views of 960x540; the 800 K-triangle dragon stand-in at depth
2, 16 views of 256x256."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402

WORKLOADS = [  # name, scene, depth, B, W, H
    ("cornell_b1_256", "cornell", 4, 1, 256, 256),
    ("cornell_b4_256", "cornell", 4, 4, 256, 256),
    ("cornell_b16_256", "cornell", 4, 16, 256, 256),
    ("cornell_b64_256", "cornell", 4, 64, 256, 256),
    ("cornell_b16_960x540", "cornell", 4, 16, 960, 540),
    ("dragon_b16_256", "dragon", 2, 16, 256, 256),
]


def cameras(pkg, B, W, H):
    """B views on a circle around the default camera's look-at point (yaw steps of 360/B degrees, a little pitch)."""
    base = pkg.scenes.default_camera(W, H).astype(np.float32)
    a = np.repeat(base[None, :], B, axis=0)
    k = np.arange(B, dtype=np.float32)
    a[:, 4] = base[4] + np.float32(2.0 * np.pi / max(B, 1)) * k
    a[:, 3] = base[3] + np.float32(0.1) * np.sin(k)
    return np.ascontiguousarray(a, np.float32)


def tile_order(W, H, tile=8):
    y, x = np.divmod(np.arange(W * H), W)
    key = ((y // tile) * ((W + tile - 1) // tile) + x // tile) * (tile * tile) + (y % tile) * tile + (x % tile)
    return np.argsort(key, kind="stable")


def scene_of(pkg, which, cache={}):  # noqa: B006  (one scene per process)
    if which not in cache:
        if which == "cornell":
            cache[which] = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
        else:
            cache[which] = pkg.scenes.make_dragon(800_000)
    return cache[which]


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
        order = tile_order(W, H)
        rays = np.concatenate([sc.generate_rays(c, W, H).view(np.float32).reshape(-1, 7)[order] for c in cams])
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
        out_views = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        out_single = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        out_list = torch.empty((B * W * H, 3), dtype=torch.float32, device=dev)

        def views():
            return [sc.render_views_tensor(cams, W, H, out=out_views, max_level=depth)[1]]

        def singles(predict):
            pkg.set_render_prediction(predict)
            st = [sc.render_tensor(cams[b], W, H, out=out_single[b], max_level=depth)[1] for b in range(B)]
            pkg.set_render_prediction(True)
            return st

        def listed():
            return [sc.shade_rays_tensor(d_rays, out=out_list, max_level=depth)[1]]

        routes = {"views": views, "exact": lambda: singles(False), "predicted": lambda: singles(True), "list": listed}
        if a.kernels:
            for _ in range(5):
                for fn in routes.values():
                    fn()
            torch.cuda.synchronize()
            print("kernels run done:", name)
            sc.close()
            continue
        for fn in routes.values():  # warm-up: workspaces grown, prediction records made
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
                samples[k]["device_ms"].append(float(sum(s["device_ms"] for s in st)))
        r = {"workload": name, "scene": which, "depth": depth, "B": B, "W": W, "H": H}
        for k, v in samples.items():
            r[k] = {"call_ms": float(np.median(v["call_ms"])), "call_ms_min": float(np.min(v["call_ms"])), "device_ms": float(np.median(v["device_ms"]))}
        r["speedup_call_vs_exact"] = r["exact"]["call_ms"] / r["views"]["call_ms"]
        r["speedup_call_vs_predicted"] = r["predicted"]["call_ms"] / r["views"]["call_ms"]
        singles(False)
        torch.cuda.synchronize()
        r["views_bit_identical"] = bool(torch.equal(out_views.view(torch.int32), out_single.view(torch.int32)))
        results["runs"].append(r)
        print(json.dumps(r), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

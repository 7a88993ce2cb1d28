"""Enqueued frames (Scene.enqueue_*, include/cgrt.h cgrt_enqueue_*) against the blocking routes, in one process,
the order of the routes rotated from repeat to repeat.  Per route and workload, the median over the repeats (after warm-up) of:
  device_ms   the frame's device time from events on its stream (blocking: CgrtRenderStats.device_ms; enqueued: enqueue_stats);
  host_ms     host time of the call itself (blocking: the whole frame; enqueued: until the call returns);
  orbit_ms    wall time per frame of a 64-frame orbit loop (a new camera every frame, one synchronize at the end).
Routes: frame workloads -- predicted (render_tensor, prediction on), exact (render_tensor, prediction off), enqueued; views -- blocking
(render_views_tensor), enqueued; ray list -- blocking (shade_rays_tensor), enqueued.  The enqueued outputs are checked bit for bit against
the blocking ones.  The cap of the count-driven grids is read once per process from CGRT_STRIDED_WAVES (default 6144 waves).

  python3 tools/measure_enqueue.py [--repeats N] [--out FILE.json] [--only NAME]
  python3 tools/measure_enqueue.py --kernels      (a few enqueued Cornell frames only: run under rocprofv3 --kernel-trace --stats)"""
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

WORKLOADS = [  # name, scene, kind, depth, W, H, B
    ("cornell_1080p_d4", "cornell", "frame", 4, 1920, 1080, 1),
    ("dragon800k_1080p_d2", "dragon", "frame", 2, 1920, 1080, 1),
    ("cornell_views16_256_d4", "cornell", "views", 4, 256, 256, 16),
    ("cornell_list_1080p_d2", "cornell", "list", 2, 1920, 1080, 1),
]


def orbit(pkg, W, H, i, n=64):
    cam = pkg.scenes.default_camera(W, H).astype(np.float32).copy()
    cam[4] += np.float32(0.02 * np.sin(2 * np.pi * i / n))
    cam[3] += np.float32(0.01 * np.cos(2 * np.pi * i / n))
    return cam


def views_of(pkg, B, W, H, shift=0):
    return np.stack([orbit(pkg, W, H, shift + k, 16) for k in range(B)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enqueue_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    pkg = entry.load_package()
    cache = {}

    def scene(which):
        if which not in cache:
            sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz")) if which == "cornell"
                  else pkg.scenes.make_dragon(800_000))
            cache[which] = pkg.Scene(sd, device=0)
        return cache[which]

    if a.kernels:  # one warm enqueued Cornell frame per iteration, for the kernel trace
        sc = scene("cornell")
        cam = pkg.scenes.default_camera(1920, 1080)
        out = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
        for _ in range(4):
            sc.enqueue_render_tensor(cam, 1920, 1080, out=out, max_level=4)
        torch.cuda.synchronize()
        print("kernels: 4 enqueued Cornell 1080p depth-4 frames")
        return
    results = {"strided_waves": int(os.environ.get("CGRT_STRIDED_WAVES", "6144")), "repeats": a.repeats, "workloads": {}}
    for name, which, kind, depth, W, H, B in WORKLOADS:
        if a.only and a.only not in name:
            continue
        sc = scene(which)
        if kind == "list":
            rays = torch.from_numpy(np.ascontiguousarray(sc.generate_rays(pkg.scenes.default_camera(W, H), W, H)).view(np.float32).reshape(H, W, 7).copy()).cuda()
            shape = (H, W, 3)
        elif kind == "views":
            shape = (B, H, W, 3)
        else:
            shape = (H, W, 3)
        out_b = torch.empty(shape, dtype=torch.float32, device="cuda")
        out_e = torch.empty(shape, dtype=torch.float32, device="cuda")

        def blocking(i, route):
            pkg.set_render_prediction(route != "exact")
            if kind == "frame":
                return sc.render_tensor(orbit(pkg, W, H, i), W, H, out=out_b, max_level=depth)[1]
            if kind == "views":
                return sc.render_views_tensor(views_of(pkg, B, W, H, i), W, H, out=out_b, max_level=depth)[1]
            return sc.shade_rays_tensor(rays, out=out_b, max_level=depth)[1]

        def enqueued(i, out=None):
            out = out_e if out is None else out
            if kind == "frame":
                return sc.enqueue_render_tensor(orbit(pkg, W, H, i), W, H, out=out, max_level=depth)[1]
            if kind == "views":
                return sc.enqueue_render_views_tensor(views_of(pkg, B, W, H, i), W, H, out=out, max_level=depth)[1]
            return sc.enqueue_shade_rays_tensor(rays, out=out, max_level=depth)[1]

        routes = ["predicted", "exact", "enqueued"] if kind == "frame" else ["blocking", "enqueued"]
        # warm-up, and the bit check
        for i in range(3):
            for r in routes:
                if r != "enqueued":
                    blocking(0, r)
            enqueued(0)
        torch.cuda.synchronize()
        blocking(0, routes[0])
        torch.cuda.synchronize()
        identical = bool(torch.equal(out_b.view(torch.int32), out_e.view(torch.int32)))
        samples = {r: {"device_ms": [], "host_ms": [], "orbit_ms": []} for r in routes}
        outs = [torch.empty(shape, dtype=torch.float32, device="cuda") for _ in range(4)]
        for rep in range(a.repeats):
            order = routes[rep % len(routes):] + routes[:rep % len(routes)]
            for r in order:
                if r == "predicted":
                    blocking(rep, r)  # (the exact route switched prediction off: the next frame re-learns the counts)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if r == "enqueued":
                    t = enqueued(rep)
                    host = time.perf_counter() - t0
                    dev = sc.enqueue_stats(t)["device_ms"]
                else:
                    st = blocking(rep, r)
                    host = time.perf_counter() - t0
                    dev = st["device_ms"]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(64):
                    if r == "enqueued":
                        enqueued(i, outs[i % 4])
                    else:
                        blocking(i, r)
                torch.cuda.synchronize()
                orb = (time.perf_counter() - t0) / 64
                samples[r]["device_ms"].append(dev)
                samples[r]["host_ms"].append(host * 1e3)
                samples[r]["orbit_ms"].append(orb * 1e3)
        pkg.set_render_prediction(True)
        med = {r: {k: float(np.median(v)) for k, v in d.items()} for r, d in samples.items()}
        results["workloads"][name] = {"scene": which, "kind": kind, "depth": depth, "W": W, "H": H, "views": B, "bit_identical": identical,
                                      "median": med}
        print(name, "identical" if identical else "DIFFERENT", json.dumps(med))
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Ray lists through the shading wavefront (cgrt_shade_rays_device via Scene.shade_rays_tensor) against the camera's own frame
(Scene.render_tensor), on the same rays: the camera's 1920x1080 rays from generate_rays, in row-major order and re-ordered into 8x8
tiles.  The frame is timed on its exactly sized path (prediction off) and on its predicted path.  Per configuration: median of the
repeats (after warm-up) of the whole call up to a synchronize, and of the library's own device time (stats device_ms).

  python3 tools/measure_shade_rays.py [--repeats N] [--out FILE.json] [--only cornell|dragon]
  python3 tools/measure_shade_rays.py --kernels row|tiled     (a few calls only: run under rocprofv3 --kernel-trace --stats)

Scenes: Cornell and the 800 K-triangle dragon stand-in of tools/measure_aa.py, depths 2 and 4."""
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

W, H = 1920, 1080


def scenes(pkg, only):
    out = []
    if only in (None, "cornell"):
        out.append(("cornell", pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))))
    if only in (None, "dragon"):
        out.append(("dragon800k", pkg.scenes.make_dragon(800_000)))
    return out


def tile_order(W, H, tile=8):
    """Pixel indices y*W + x in 8x8-tile order: tiles row-major, pixels row-major inside a tile."""
    y, x = np.divmod(np.arange(W * H), W)
    key = ((y // tile) * ((W + tile - 1) // tile) + x // tile) * (tile * tile) + (y % tile) * tile + (x % tile)
    return np.argsort(key, kind="stable")


def timed(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, dev = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        st = fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(st["device_ms"])
    return dict(call_ms=float(np.median(wall)), device_ms=float(np.median(dev)), call_ms_min=float(np.min(wall)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kernels", default=None, choices=("row", "tiled"))
    a = ap.parse_args()
    pkg = entry.load_package()
    sd = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
    if a.kernels:  # a short run for the kernel trace: the list kernel and, for the same rays, the frame's primary kernel (exact path)
        sc = pkg.Scene(sd, device=0)
        cam = pkg.scenes.default_camera(W, H)
        rays = sc.generate_rays(cam, W, H).view(np.float32).reshape(-1, 7)
        if a.kernels == "tiled":
            rays = rays[tile_order(W, H)]
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
        out = torch.empty((W * H, 3), device="cuda:0")
        pkg.set_render_prediction(False)
        for _ in range(10):
            sc.shade_rays_tensor(d_rays, out=out, max_level=2)
            sc.render_tensor(cam, W, H, max_level=2)
        torch.cuda.synchronize()
        print("kernels run done:", a.kernels)
        return
    results = {"W": W, "H": H, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "source_hash": pkg.source_hash(), "runs": []}
    order = tile_order(W, H)
    for name, s in scenes(pkg, a.only):
        sc = pkg.Scene(s, device=0)
        cam = pkg.scenes.default_camera(W, H)
        rays = sc.generate_rays(cam, W, H).view(np.float32).reshape(-1, 7)
        d_row = torch.from_numpy(rays).to("cuda:0")
        d_tiled = torch.from_numpy(np.ascontiguousarray(rays[order])).to("cuda:0")
        out = torch.empty((W * H, 3), device="cuda:0")
        frame = torch.empty((H, W, 3), device="cuda:0")
        for depth in (2, 4):
            r = {"scene": name, "depth": depth}
            pkg.set_render_prediction(False)
            r["frame_exact"] = timed(lambda: sc.render_tensor(cam, W, H, out=frame, max_level=depth)[1], a.repeats)
            pkg.set_render_prediction(True)
            r["frame_predicted"] = timed(lambda: sc.render_tensor(cam, W, H, out=frame, max_level=depth)[1], a.repeats)
            r["frame_predicted_path"] = sc.last_render_path()
            want = frame.cpu().numpy().reshape(-1, 3)
            r["list_row_major"] = timed(lambda: sc.shade_rays_tensor(d_row, out=out, max_level=depth)[1], a.repeats)
            r["row_major_bit_identical"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)))
            r["list_tiled"] = timed(lambda: sc.shade_rays_tensor(d_tiled, out=out, max_level=depth)[1], a.repeats)
            r["tiled_bit_identical"] = bool(np.array_equal(out.cpu().numpy().view(np.uint32), want[order].view(np.uint32)))
            results["runs"].append(r)
            print(json.dumps(r), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

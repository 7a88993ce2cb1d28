"""Geometry buffers of a device frame (Scene.render_aov_tensor) against what a caller did before them: the frame,
then a second primary trace into a hit buffer and a normals buffer.  Warm frames of one camera, every route timed frame by frame on the
host clock up to a device synchronise, the routes taken in turn (rotated from frame to frame); per route the median and the quartiles.

Routes, on (a) Cornell 1920 x 1080 depth 4 and (b) the 800 K dragon stand-in 1920 x 1080 depth 2:
  render         render_tensor alone
  render+trace   render_tensor, then trace_primary_device into hits + normals (depth / ids / mask / normal the old way)
  aov5           render_aov_tensor with depth, normal, prim_id, material_id, mask      (libraries that have the entry)
  aov7           render_aov_tensor with all seven planes                               (libraries that have the entry)
--package DIR measures another checkout's package directory (its own libcgrt.so) with this script -- the parent commit, which has no
geometry buffers and runs the first two routes only.  Run the two checkouts in turn, each in a process of its own.

  python3 tools/measure_aov.py [--frames N] [--package DIR] [--label NAME] [--out FILE.json] [--only NAME] [--routes a,b]
  python3 tools/measure_aov.py --kernels     (20 aov7 and 20 aov5 frames of both workloads: run under rocprofv3 --kernel-trace --stats)

The export's traffic model, printed with the results: the fill writes 49 B per pixel for all seven planes (4 + 12 + 12 + 12 + 4 + 4 + 1;
25 B for the five), the scatter reads 60 B per level-0 entry (28 ray + 16 hit + 12 normal + 4 pixel) and writes the same 49 (25) B again."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402

WORKLOADS = [("cornell_1080p_d4", "cornell", 4, 1920, 1080), ("dragon800k_1080p_d2", "dragon", 2, 1920, 1080)]
FIVE = ("depth", "normal", "prim_id", "material_id", "mask")
PLANE_BYTES = {"depth": 4, "normal": 12, "position": 12, "albedo": 12, "prim_id": 4, "material_id": 4, "mask": 1}


def load_package(path):
    if not path:
        return entry.load_package()
    path = os.path.abspath(path)
    spec = importlib.util.spec_from_file_location("cg_raytracer_amd_other", os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["cg_raytracer_amd_other"] = mod
    spec.loader.exec_module(mod)
    return mod


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": float(med), "q1_ms": float(q1), "q3_ms": float(q3), "iqr_ms": float(q3 - q1), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--package")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out")
    ap.add_argument("--only")
    ap.add_argument("--routes", help="comma-separated subset of the routes (the routes of a process share the caches: compare like with like)")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_aov.py needs a GPU: a time taken elsewhere says nothing")
    pkg = load_package(a.package)
    has_aov = hasattr(pkg.Scene, "render_aov_tensor")
    results = {"label": a.label, "frames": a.frames, "source_hash": pkg.source_hash(), "workloads": {}}
    for name, which, depth, W, H in WORKLOADS:
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz")) if which == "cornell"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        cam = pkg.scenes.default_camera(W, H)
        out = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        hits = torch.empty((W * H * 16,), dtype=torch.uint8, device="cuda")
        normals = torch.empty((W * H * 12,), dtype=torch.uint8, device="cuda")
        planes = {}
        if has_aov:
            dt = {"prim_id": torch.int32, "material_id": torch.int32, "mask": torch.uint8}
            planes = {k: torch.empty((H, W, 3) if b == 12 else (H, W), dtype=dt.get(k, torch.float32), device="cuda") for k, b in PLANE_BYTES.items()}

        def render():
            sc.render_tensor(cam, W, H, out=out, max_level=depth)

        def render_trace():
            sc.render_tensor(cam, W, H, out=out, max_level=depth)
            sc.trace_primary_device(cam, W, H, hits.data_ptr(), d_normals_ptr=normals.data_ptr())

        def aov(names):
            return lambda: sc.render_aov_tensor(cam, W, H, aovs=names, out=out, aov_out={k: planes[k] for k in names}, max_level=depth)

        routes = {"render": render, "render+trace": render_trace}
        if has_aov:
            routes["aov5"] = aov(FIVE)
            routes["aov7"] = aov(tuple(PLANE_BYTES))
        if a.routes:
            routes = {r: routes[r] for r in a.routes.split(",")}
        if a.kernels:
            for r in ("aov7", "aov5"):
                for _ in range(20):
                    routes[r]()
            torch.cuda.synchronize()
            print("kernels:", name, "20 frames each of aov7 and aov5")
            sc.close()
            continue
        order = list(routes)
        for _ in range(20):  # warm: code objects, the workspace, the prediction record
            for r in order:
                routes[r]()
        torch.cuda.synchronize()
        samples = {r: [] for r in order}
        for i in range(a.frames):
            k = i % len(order)
            for r in order[k:] + order[:k]:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                routes[r]()
                torch.cuda.synchronize()
                samples[r].append((time.perf_counter() - t0) * 1e3)
        res = {r: quartiles(v) for r, v in samples.items()}
        st = sc.render_tensor(cam, W, H, out=out, max_level=depth)[1]
        torch.cuda.synchronize()
        entries = None  # (level 0's entries: the mask's sum, where the library has the planes)
        if has_aov:
            m = sc.render_aov_tensor(cam, W, H, aovs=("mask",), out=out, aov_out={"mask": planes["mask"]}, max_level=depth)[2]["mask"]
            torch.cuda.synchronize()
            entries = int(m.sum().item())
        model = {n: {"fill_bytes": b * W * H, "scatter_read_bytes": 60 * entries, "scatter_write_bytes": b * entries}
                 for n, b in (("aov5", sum(PLANE_BYTES[k] for k in FIVE)), ("aov7", sum(PLANE_BYTES.values())))} if has_aov else None
        results["workloads"][name] = {"scene": which, "depth": depth, "W": W, "H": H, "render_path": sc.last_render_path(),
                                      "level0_entries": entries, "routes": res, "bytes_model": model}
        print(a.label, name, "entries", entries, json.dumps(res))
        sc.close()
    if a.out and not a.kernels:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Multi-view light sets (Scene.render_views_light_sets_tensor, cgrt_render_views_light_sets_device) against the two single-axis batch
families a caller has without them, in the same process, the order of the routes rotated from repeat to repeat:
  batch       ONE render_views_light_sets_tensor call for the V cameras and S light sets;
  per_camera  V render_light_sets_tensor calls (one per camera, each with the S sets);
  per_set     S render_views_tensor calls (one per set, each with the V cameras).
Per route: median over the repeats of the host time of the whole route up to a synchronize, and of the library's device_ms (summed over the
calls of a route).  The batch's frames are checked bit for bit against both routes' frames.  Then an orbit loop: 64 enqueued batches
(enqueue_render_views_light_sets_tensor), the cameras turning from batch to batch, two output buffers in turn: wall time per batch, the
median host time of one call, and the median of the tickets' device_ms.

  python3 tools/measure_views_light_sets.py [--repeats N] [--out FILE.json] [--only NAME]
  python3 tools/measure_views_light_sets.py --kernels NAME     (a few batches only: run under rocprofv3 --kernel-trace --stats)

Workloads: Cornell 256x256 at depth 4, V = S = 16, as a colour sweep and as a position sweep of its light; Cornell 1920x1080 at depth 4,
V = S = 4 (colour sweep).  The orbit loop runs the 256x256 colour sweep."""
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

WORKLOADS = [  # name, depth, V, S, W, H, sweep
    ("cornell_colour_v16_s16_256", 4, 16, 16, 256, 256, "colour"),
    ("cornell_position_v16_s16_256", 4, 16, 16, 256, 256, "position"),
    ("cornell_colour_v4_s4_1080p", 4, 4, 4, 1920, 1080, "colour"),
]
ORBIT = ("cornell_orbit_v16_s16_256", 4, 16, 16, 256, 256, "colour", 64)


def light_sets(sd, S, sweep):
    L = np.ascontiguousarray(np.asarray(sd.point_lights, np.float32).reshape(-1, 6))
    k = np.arange(S, dtype=np.float32)
    sets = []
    for s in range(S):
        x = L.copy()
        if sweep == "colour":
            x[:, 3:6] *= np.float32(0.2) + np.float32(0.05) * k[s]
        else:
            x[:, 0:3] += np.float32([0.02, -0.01, 0.015]) * k[s]
        sets.append(x)
    return sets


def cameras(pkg, V, W, H, turn=0.0):
    """V cameras on an arc around the default one (euler x), the arc turned by `turn`"""
    base = pkg.scenes.default_camera(W, H).astype(np.float32)
    a = np.repeat(base[None, :], V, axis=0)
    a[:, 4] += np.float32(turn) + np.float32(0.03) * np.arange(V, dtype=np.float32)
    return np.ascontiguousarray(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kernels", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    results = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "source_hash": pkg.source_hash(), "runs": []}
    sd = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
    for name, depth, V, S, W, H, sweep in WORKLOADS:
        if (a.only and name != a.only) or (a.kernels and name != a.kernels):
            continue
        sc = pkg.Scene(sd, device=0)
        cams = cameras(pkg, V, W, H)
        sets = light_sets(sd, S, sweep)
        out_b = torch.empty((V, S, H, W, 3), dtype=torch.float32, device=dev)
        out_c = torch.empty((V, S, H, W, 3), dtype=torch.float32, device=dev)  # per camera: out_c[v] = (S, H, W, 3)
        out_s = torch.empty((S, V, H, W, 3), dtype=torch.float32, device=dev)  # per set: out_s[s] = (V, H, W, 3)

        def batch():
            return [sc.render_views_light_sets_tensor(cams, W, H, sets, out=out_b, max_level=depth)[1]]

        def per_camera():
            return [sc.render_light_sets_tensor(cams[v], W, H, sets, out=out_c[v], max_level=depth)[1] for v in range(V)]

        def per_set():
            return [sc.render_views_tensor(cams, W, H, out=out_s[s], lights=sets[s], max_level=depth)[1] for s in range(S)]

        routes = {"batch": batch, "per_camera": per_camera, "per_set": per_set}
        if a.kernels:
            for _ in range(3):
                batch()
            torch.cuda.synchronize()
            print("kernels run done:", name)
            sc.close()
            continue
        for fn in routes.values():  # warm-up: workspaces grown
            for _ in range(2):
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
        r = {"workload": name, "scene": "cornell", "depth": depth, "V": V, "S": S, "W": W, "H": H, "sweep": sweep}
        for k, v in samples.items():
            r[k] = {"call_ms": float(np.median(v["call_ms"])), "call_ms_min": float(np.min(v["call_ms"])), "device_ms": float(np.median(v["device_ms"]))}
        faster = min(r["per_camera"]["call_ms"], r["per_set"]["call_ms"])
        r["speedup_call_vs_per_camera"] = r["per_camera"]["call_ms"] / r["batch"]["call_ms"]
        r["speedup_call_vs_per_set"] = r["per_set"]["call_ms"] / r["batch"]["call_ms"]
        r["passes_bar"] = r["batch"]["call_ms"] <= faster
        st_b = batch()[0]
        st_c = per_camera()
        per_set()
        torch.cuda.synchronize()
        r["stats_batch"] = {k: st_b[k] for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels")}
        r["stats_per_camera_sum"] = {k: int(sum(s[k] for s in st_c)) for k in ("primary_rays", "shadow_rays", "reflection_rays")}
        r["bit_identical_per_camera"] = bool(torch.equal(out_b.view(torch.int32), out_c.view(torch.int32)))
        r["bit_identical_per_set"] = bool(torch.equal(out_b.view(torch.int32), out_s.transpose(0, 1).contiguous().view(torch.int32)))
        results["runs"].append(r)
        print(json.dumps(r), flush=True)
        sc.close()
    name, depth, V, S, W, H, sweep, N = ORBIT
    if not a.kernels and (not a.only or a.only == name):
        sc = pkg.Scene(sd, device=0)
        sets = light_sets(sd, S, sweep)
        outs = [torch.empty((V, S, H, W, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        ref = torch.empty_like(outs[0])
        for i in range(3):  # warm-up: workspace and ticket slots
            sc.enqueue_render_views_light_sets_tensor(cameras(pkg, V, W, H, 0.01 * i), W, H, sets, out=outs[i % 2], max_level=depth)
        torch.cuda.synchronize()
        loops = []
        for rep in range(3):
            call_ms, tickets = [], []
            t0 = time.perf_counter()
            for i in range(N):
                c = cameras(pkg, V, W, H, 0.01 * i)
                t1 = time.perf_counter()
                _, t = sc.enqueue_render_views_light_sets_tensor(c, W, H, sets, out=outs[i % 2], max_level=depth)
                call_ms.append((time.perf_counter() - t1) * 1e3)
                tickets.append(t)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            dev_ms = [sc.enqueue_stats(t)["device_ms"] for t in tickets[-8:]]  # (the ticket ring holds the last 8 batches)
            loops.append({"wall_ms_per_batch": wall / N, "call_ms_median": float(np.median(call_ms)), "device_ms_median": float(np.median(dev_ms))})
        sc.render_views_light_sets_tensor(cameras(pkg, V, W, H, 0.01 * (N - 1)), W, H, sets, out=ref, max_level=depth)
        torch.cuda.synchronize()
        r = {"workload": name, "scene": "cornell", "depth": depth, "V": V, "S": S, "W": W, "H": H, "sweep": sweep, "batches": N,
             "wall_ms_per_batch": float(np.median([x["wall_ms_per_batch"] for x in loops])),
             "call_ms_median": float(np.median([x["call_ms_median"] for x in loops])),
             "device_ms_median": float(np.median([x["device_ms_median"] for x in loops])),
             "last_batch_bit_identical": bool(torch.equal(outs[(N - 1) % 2].view(torch.int32), ref.view(torch.int32))), "loops": loops}
        results["runs"].append(r)
        print(json.dumps(r), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

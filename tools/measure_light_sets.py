"""Light sets (Scene.render_light_sets_tensor, cgrt_render_light_sets_device) against the routes a caller has without them, in the same
process, the order of the routes rotated from repeat to repeat:
  sets        ONE render_light_sets_tensor call for the B light sets;
  exact       B render_tensor calls on one stream, prediction off (the exactly sized path every batch takes);
  predicted   B render_tensor calls, prediction on (the scene's previous frame of the shape sizes the next: the single frame's fastest path).
Per route: median over the repeats of the host time of the whole batch up to a synchronize, and of the library's device_ms (summed over
the calls of a route).  The sets' frames are checked bit for bit against the exact route's.

  python3 tools/measure_light_sets.py [--repeats N] [--out FILE.json] [--only NAME]
  python3 tools/measure_light_sets.py --kernels NAME     (a few batches only: run under rocprofv3 --kernel-trace --stats)

Workloads: Cornell 1920x1080 at depth 4, a colour sweep of its lights with B = 1, 4, 16 and a position sweep with B = 16; the 800 K-triangle
dragon stand-in at 1920x1080, depth 2, a colour sweep with B = 8; Cornell at 960x540, depth 4, a sweep of a spherical light's position with
B = 4 (samples 16)."""
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

WORKLOADS = [  # name, scene, depth, B, W, H, sweep
    ("cornell_colour_b1_1080p", "cornell", 4, 1, 1920, 1080, "colour"),
    ("cornell_colour_b4_1080p", "cornell", 4, 4, 1920, 1080, "colour"),
    ("cornell_colour_b16_1080p", "cornell", 4, 16, 1920, 1080, "colour"),
    ("cornell_position_b16_1080p", "cornell", 4, 16, 1920, 1080, "position"),
    ("dragon_colour_b8_1080p", "dragon", 2, 8, 1920, 1080, "colour"),
    ("cornell_spherical_b4_960x540", "cornell", 4, 4, 960, 540, "spherical"),
]
SAMPLES = 16


def light_sets(pkg, sd, B, sweep):
    """(point-light sets, spherical sets or None): the scene's lights recoloured, moved, or with one spherical light moved"""
    L = np.ascontiguousarray(np.asarray(sd.point_lights, np.float32).reshape(-1, 6))
    k = np.arange(B, dtype=np.float32)
    sets, sph = [], None
    for b in range(B):
        x = L.copy()
        if sweep == "colour":
            x[:, 3:6] *= np.float32(0.2) + np.float32(0.05) * k[b]
        elif sweep == "position":
            x[:, 0:3] += np.float32([0.02, -0.01, 0.015]) * k[b]
        sets.append(x)
    if sweep == "spherical":
        sph = []
        for b in range(B):
            y = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
            y[:, 0:3] += np.float32([0.03, 0.0, -0.02]) * k[b]
            sph.append(y)
    return sets, sph


def scene_of(pkg, which, cache={}):  # noqa: B006  (one scene per process)
    if which not in cache:
        if which == "cornell":
            cache[which] = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
        else:
            cache[which] = pkg.scenes.make_dragon(800_000)
    return cache[which]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kernels", default=None)
    a = ap.parse_args()
    pkg = entry.load_package()
    dev = torch.device("cuda", 0)
    results = {"repeats": a.repeats, "device": torch.cuda.get_device_name(0), "source_hash": pkg.source_hash(), "runs": []}
    for name, which, depth, B, W, H, sweep in WORKLOADS:
        if (a.only and name != a.only) or (a.kernels and name != a.kernels):
            continue
        sd = scene_of(pkg, which)
        sc = pkg.Scene(sd, device=0)
        cam = pkg.scenes.default_camera(W, H)
        sets, sph = light_sets(pkg, sd, B, sweep)
        units = pkg.unit_vector_table(1 << 16, 0)
        soft = dict(units=units, samples=SAMPLES, seed=0) if sph is not None else {}
        out_sets = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
        out_single = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)

        def batch():
            return [sc.render_light_sets_tensor(cam, W, H, sets, out=out_sets, max_level=depth, spherical_sets=sph, **soft)[1]]

        def singles(predict):
            pkg.set_render_prediction(predict)
            st = []
            for b in range(B):
                kw = dict(spherical=sph[b], **soft) if sph is not None else {}
                st.append(sc.render_tensor(cam, W, H, out=out_single[b], lights=sets[b], max_level=depth, **kw)[1])
            pkg.set_render_prediction(True)
            return st

        routes = {"sets": batch, "exact": lambda: singles(False), "predicted": lambda: singles(True)}
        if a.kernels:
            for _ in range(3):
                batch()
            torch.cuda.synchronize()
            print("kernels run done:", name)
            sc.close()
            continue
        for fn in routes.values():  # warm-up: workspaces grown, prediction records made
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
        r = {"workload": name, "scene": which, "depth": depth, "B": B, "W": W, "H": H, "sweep": sweep}
        for k, v in samples.items():
            r[k] = {"call_ms": float(np.median(v["call_ms"])), "call_ms_min": float(np.min(v["call_ms"])), "device_ms": float(np.median(v["device_ms"]))}
        r["speedup_call_vs_exact"] = r["exact"]["call_ms"] / r["sets"]["call_ms"]
        r["speedup_call_vs_predicted"] = r["predicted"]["call_ms"] / r["sets"]["call_ms"]
        st_sets = batch()[0]
        st_exact = singles(False)
        torch.cuda.synchronize()
        r["stats_sets"] = {k: st_sets[k] for k in ("shadow_rays", "reflection_rays", "soft_shadow_rays")}
        r["stats_exact_sum"] = {k: int(sum(s[k] for s in st_exact)) for k in ("shadow_rays", "reflection_rays", "soft_shadow_rays")}
        r["sets_bit_identical"] = bool(torch.equal(out_sets.view(torch.int32), out_single.view(torch.int32)))
        results["runs"].append(r)
        print(json.dumps(r), flush=True)
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()

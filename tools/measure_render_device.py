"""Shaded frames into device memory (cgrt_render_device) against the pinned-host entries (cgrt_render_mapped / cgrt_render_aa_mapped):
per predicted frame, the HIP-event time of the frame's kernels (stats device_ms, the export not included), the wall time of the mapped
C call (no copy after it), the wall time of Scene.render_device (raw pointer) into a torch tensor on the current stream up to a
torch.cuda.synchronize(), and the same for Scene.render_tensor (a new tensor per frame, the current stream), for each format.  Medians over --repeats predicted frames after --warmup frames, a fresh scene per row.
Scenes: Cornell 1920x1080 depth 4 and the 800 K dragon stand-in depth 2, plain and anti-aliased.
  python3 tools/measure_render_device.py [--repeats N] [--warmup N] [--out FILE.json] [--only cornell|dragon]
  python3 tools/measure_render_device.py --frames N   (N device frames per format and mode of the first scene, nothing printed: for a
                                                      rocprofv3 --kernel-trace --stats run, which gives k_export_frame's kernel time)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as e  # noqa: E402

pkg = e.load_package()
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "scenes")
FORMATS = ("rgb", "chw", "rgba8")


def scenes(only):
    out = []
    if only in (None, "cornell"):
        out.append(("cornell", pkg.scenes.SceneData.load(os.path.join(GOLDEN, "cornell.npz")), 1920, 1080, 4))
    if only in (None, "dragon"):
        out.append(("dragon800k", pkg.scenes.make_dragon(800_000), 1920, 1080, 2))
    return out


def mapped_call(sc, cam, W, H, depth, aa):
    """The C entry alone (the Python wrappers copy the pinned frame afterwards): (device_ms, wall_ms, render path)."""
    lights = pkg._f32(sc.sd.point_lights, (-1, 6))
    c = pkg.Camera.from_array(cam)
    st, ptr = pkg.RenderStats(), C.c_void_p()
    f = pkg.lib().cgrt_render_aa_mapped if aa else pkg.lib().cgrt_render_mapped
    t0 = time.perf_counter()
    pkg._check(f(sc._h, C.byref(c), W, H, pkg._ptr(lights), len(lights), None, depth, C.byref(ptr), C.byref(st)))
    return st.device_ms, (time.perf_counter() - t0) * 1e3, sc.last_render_path()


def device_call(torch, sc, cam, W, H, depth, aa, fmt, out):
    t0 = time.perf_counter()
    st = sc.render_device(cam, W, H, out.data_ptr(), format=fmt, stream=torch.cuda.current_stream().cuda_stream, aa=aa, max_level=depth)
    torch.cuda.synchronize()
    return st["device_ms"], (time.perf_counter() - t0) * 1e3, sc.last_render_path()


def tensor_call(torch, sc, cam, W, H, depth, aa, fmt):
    t0 = time.perf_counter()
    _, st = sc.render_tensor(cam, W, H, format=fmt, aa=aa, max_level=depth)
    torch.cuda.synchronize()
    return st["device_ms"], (time.perf_counter() - t0) * 1e3, sc.last_render_path()


def med(rows, i):
    pred = [r[i] for r in rows if r[2] == 1]  # predicted frames only
    return (statistics.median(pred) if pred else None), len(pred)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--frames", type=int, default=0)
    a = ap.parse_args()
    import torch  # (before the library is loaded: torch brings the HIP runtime both then use)

    if pkg.device_count() < 1:
        raise SystemExit("needs a HIP device")

    outs = {}

    def out_of(fmt, W, H):
        if (fmt, W, H) not in outs:
            shape, dt = {"rgb": ((H, W, 3), torch.float32), "chw": ((3, H, W), torch.float32), "rgba8": ((H, W, 4), torch.uint8)}[fmt]
            outs[(fmt, W, H)] = torch.empty(shape, dtype=dt, device="cuda:0")
        return outs[(fmt, W, H)]

    if a.frames:
        name, sd, W, H, depth = scenes(a.only)[0]
        cam = pkg.scenes.default_camera(W, H)
        for aa in (False, True):
            sc = pkg.Scene(sd, device=0)
            for fmt in FORMATS:
                for _ in range(a.frames):
                    device_call(torch, sc, cam, W, H, depth, aa, fmt, out_of(fmt, W, H))
            sc.close()
        return
    warm = pkg.Scene(scenes("cornell")[0][1], device=0)  # the process's first launches (code objects loading) are not part of any row
    for aa in (False, True):
        for fmt in FORMATS:
            warm.render_tensor(pkg.scenes.default_camera(64, 64), 64, 64, format=fmt, aa=aa)
    torch.cuda.synchronize()
    warm.close()
    res = {}
    for name, sd, W, H, depth in scenes(a.only):
        cam = pkg.scenes.default_camera(W, H)
        r = {}
        for label, aa in (("plain", False), ("aa", True)):
            row = {}
            sc = pkg.Scene(sd, device=0)  # a fresh scene per row
            for _ in range(a.warmup):
                mapped_call(sc, cam, W, H, depth, aa)
            rows = [mapped_call(sc, cam, W, H, depth, aa) for _ in range(a.repeats)]
            row["mapped"] = dict(zip(("device_ms", "wall_ms"), (med(rows, 0)[0], med(rows, 1)[0])), predicted_frames=med(rows, 0)[1])
            for fmt in FORMATS:
                out = out_of(fmt, W, H)
                for _ in range(a.warmup):
                    device_call(torch, sc, cam, W, H, depth, aa, fmt, out)
                rows = [device_call(torch, sc, cam, W, H, depth, aa, fmt, out) for _ in range(a.repeats)]
                row[f"device_{fmt}"] = dict(zip(("device_ms", "wall_ms"), (med(rows, 0)[0], med(rows, 1)[0])), predicted_frames=med(rows, 0)[1])
                for _ in range(a.warmup):
                    tensor_call(torch, sc, cam, W, H, depth, aa, fmt)
                rows = [tensor_call(torch, sc, cam, W, H, depth, aa, fmt) for _ in range(a.repeats)]
                row[f"tensor_{fmt}"] = dict(zip(("device_ms", "wall_ms"), (med(rows, 0)[0], med(rows, 1)[0])), predicted_frames=med(rows, 0)[1])
            sc.close()
            r[label] = row
        key = f"{name} {W}x{H} depth {depth}"
        res[key] = r
        print(json.dumps({key: r}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

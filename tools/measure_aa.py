"""Plain vs anti-aliased frames of the same W x H (cgrt_render vs cgrt_render_aa, the reference's antiAliasing branch): HIP-event time of
the frame's kernels (stats device_ms) and the whole call's wall time, for the first frame of a shape (exactly sized) and for the
predicted frames that follow it (median of the repeats).  Scenes: Cornell 1920x1080 depth 4 and the 800 K dragon stand-in depth 2.
  python3 tools/measure_aa.py [--repeats N] [--out FILE.json] [--only cornell|dragon] [--frames N]
--frames N: render N AA frames of the first scene only and print nothing else (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as e  # noqa: E402

pkg = e.load_package()
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "scenes")


def scenes(only):
    out = []
    if only in (None, "cornell"):
        out.append(("cornell", pkg.scenes.SceneData.load(os.path.join(GOLDEN, "cornell.npz")), 1920, 1080, 4))
    if only in (None, "dragon"):
        out.append(("dragon800k", pkg.scenes.make_dragon(800_000), 1920, 1080, 2))
    return out


def frames(sc, cam, W, H, depth, aa, repeats):
    """[first frame, predicted frames...] as (device_ms, wall_ms, render path)."""
    rows = []
    for _ in range(1 + repeats):
        t0 = time.perf_counter()
        _, st = (sc.render_aa(cam, W, H, max_level=depth, mapped=True) if aa else sc.render_mapped(cam, W, H, max_level=depth))
        rows.append((st["device_ms"], (time.perf_counter() - t0) * 1e3, sc.last_render_path(), st))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--frames", type=int, default=0)
    a = ap.parse_args()
    if pkg.device_count() < 1:
        raise SystemExit("needs a HIP device")
    if a.frames:
        name, sd, W, H, depth = scenes(a.only)[0]
        sc = pkg.Scene(sd, device=0)
        cam = pkg.scenes.default_camera(W, H)
        for _ in range(a.frames):
            sc.render_aa(cam, W, H, max_level=depth, mapped=True)
        return
    res = {}
    warm = pkg.Scene(scenes("cornell")[0][1], device=0)  # the process's first launches (code objects loading) are not part of any frame below
    warm.render(pkg.scenes.default_camera(64, 64), 64, 64)
    warm.render_aa(pkg.scenes.default_camera(64, 64), 64, 64)
    warm.close()
    for name, sd, W, H, depth in scenes(a.only):
        cam = pkg.scenes.default_camera(W, H)
        r = {}
        for label, aa in (("plain", False), ("aa", True)):
            sc = pkg.Scene(sd, device=0)  # a fresh scene: the first frame is a first frame of its shape
            rows = frames(sc, cam, W, H, depth, aa, a.repeats)
            pred = [x for x in rows[1:] if x[2] == 1]
            st = rows[0][3]
            r[label] = dict(first_device_ms=rows[0][0], first_wall_ms=rows[0][1],
                            predicted_device_ms=statistics.median(x[0] for x in pred) if pred else None,
                            predicted_wall_ms=statistics.median(x[1] for x in pred) if pred else None,
                            predicted_frames=len(pred), primary_rays=st["primary_rays"], shadow_rays=st["shadow_rays"],
                            reflection_rays=st["reflection_rays"], levels=st["levels"])
            sc.close()
        for k in ("first_device_ms", "first_wall_ms", "predicted_device_ms", "predicted_wall_ms"):
            if r["plain"][k] and r["aa"][k]:
                r.setdefault("ratio_aa_over_plain", {})[k] = r["aa"][k] / r["plain"][k]
        res[f"{name} {W}x{H} depth {depth}"] = r
        print(json.dumps({f"{name} {W}x{H} depth {depth}": r}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""Signed distance and occupancy (Scene.sdf_tensor, Scene.sdf_grid_tensor): the fused kernel against the Python
compositions it replaces (Scene.signed_distance_tensor / Scene.inside_tensor, unchanged since the parent commit) on the same points.

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Per scene
  list   1 048 576 points uniform in the scene box grown by 25 % (tests/closest_ref.py uniform_queries)
  grid   128^3 points over the same box; the composition is given the grid's points as a ready tensor (sdf_grid_points, not timed)
each with the distance wanted (fused sdf + inside against signed_distance_tensor) and occupancy only (fused inside against
inside_tensor); for the grid the brick lane mapping (a wave = a 4 x 4 x 4 brick) against the linear one (lanes follow the result index).

Every route writes into preallocated tensors where it can, is warmed first, and is timed between HIP events on the current stream; the
routes of a row ALTERNATE within each repetition, so that a drift of the machine hits them alike.  A row holds the median and quartiles
of every route, `spread` = (q3 - q1) / median of the fused route (the run-to-run spread), whether the fused bytes equal the composition's
on every finite point, and the direction walks run per point (debug_sdf_work on 65 536 points at most, a counting launch, not timed).
`fused_not_slower` is fused median <= composition median.  No time is asserted.

  python3 tools/measure_sdf.py [--reps N] [--out profiles/sdf_measure.json] [--only NAME] [--n POINTS] [--side N]
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


def timed(reps, routes):
    """routes: name -> call.  Medians and quartiles in ms, the routes alternating within each repetition."""
    for _ in range(3):  # warm: the code objects, torch's allocator, the caches
        for call in routes.values():
            call()
    torch.cuda.synchronize()
    events = {k: [] for k in routes}
    for _ in range(reps):
        for k, call in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, ev in events.items():
        q1, med, q3 = np.percentile([e0.elapsed_time(e1) for e0, e1 in ev], [25, 50, 75])
        out[k] = {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4)}
    return out


def same_on_finite(got, want, finite):
    g, w = got.cpu().numpy()[finite], want.cpu().numpy()[finite]
    if g.dtype == np.float32:
        return bool((g.view(np.uint32) == w.view(np.uint32)).all())
    return bool((g == w).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--side", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_sdf.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    set_mapping = lambda linear: pkg._check(pkg.lib().cgrt_debug_set_sdf_grid_mapping(linear))  # noqa: E731
    rows = []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        lo, hi = cr.scene_box(sd)
        ext = np.maximum(hi - lo, 1e-3)
        origin, spacing, dims = lo - 0.25 * ext, 1.5 * ext / (a.side - 1), (a.side,) * 3
        shapes = {"list": cr.uniform_queries(sd, a.n, 7), "grid": pkg.sdf_grid_points(origin, spacing, dims)}
        for shape, pts in shapes.items():
            n = len(pts)
            d_pts = torch.from_numpy(pts).cuda()
            finite = np.isfinite(pts).all(axis=1)
            o_s = torch.empty((n,), dtype=torch.float32, device="cuda")
            o_i = torch.empty((n,), dtype=torch.bool, device="cuda")
            m = min(n, 65536)
            sub = pts[:: n // m][:m]
            for want_sdf in (True, False):
                want = ("sdf", "inside") if want_sdf else ("inside",)
                out = (o_s, o_i) if want_sdf else o_i
                comp = (lambda: sc.signed_distance_tensor(d_pts)) if want_sdf else (lambda: sc.inside_tensor(d_pts))
                if shape == "list":
                    routes = {"fused": lambda: sc.sdf_tensor(d_pts, want=want, out=out), "composition": comp}
                else:
                    g_s, g_i = o_s.view(dims[::-1]), o_i.view(dims[::-1])
                    g_out = (g_s, g_i) if want_sdf else g_i

                    def grid_call(linear):
                        set_mapping(linear)
                        sc.sdf_grid_tensor(origin, spacing, dims, want=want, out=g_out)

                    routes = {"fused": lambda: grid_call(0), "fused_linear_mapping": lambda: grid_call(1), "composition": comp}
                t = timed(a.reps, routes)
                set_mapping(0)
                routes["fused"]()
                ref = comp()
                torch.cuda.synchronize()
                work = sc.debug_sdf_work(sub, want_sdf=want_sdf)
                row = {"scene": name, "triangles": int(sd.ntris), "shape": shape, "points": n, "want_sdf": want_sdf, **t,
                       "spread": round((t["fused"]["q3_ms"] - t["fused"]["q1_ms"]) / t["fused"]["median_ms"], 4),
                       "fused_not_slower": t["fused"]["median_ms"] <= t["composition"]["median_ms"],
                       "speedup": round(t["composition"]["median_ms"] / t["fused"]["median_ms"], 3),
                       "same_bytes_on_finite_points": same_on_finite(o_s if want_sdf else o_i, ref, finite),
                       "walks_per_point": round(work[4] / m, 4),
                       "work_per_point": {"closest_node_steps": round(work[0] / m, 2), "closest_triangles": round(work[1] / m, 2),
                                          "crossing_node_steps": round(work[2] / m, 2), "crossing_triangles": round(work[3] / m, 2)}}
                if shape == "grid":
                    row["brick_over_linear"] = round(t["fused"]["median_ms"] / t["fused_linear_mapping"]["median_ms"], 3)
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

"""Poisson-disk sets (Scene.poisson_disk_tensor): what a selection costs, and the hashed grid against the brute form.

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Candidates: stratified surface samples (Scene.sample_surface_tensor, strata =
n) under seed 1, filtered under the same seed; min_dist2 = k A / (pi n), so that a candidate has about k conflicts (A the scene's area).

  * 1 048 576 candidates, k in {8, 64}: the device form with a preallocated mask and workspace.  The call blocks, so it is timed on the
    host's clock between a device synchronisation and its return; medians and quartiles of --reps calls after three warm ones.  The split
    into grid build and rounds, the rounds, the pair tests and the buckets come from cgrt_debug_poisson_work (the counted kernels, a
    wait for the stream between the parts; median of five runs), so build + rounds is not the total.
  * 65 536 candidates, k in {8, 64}: the host form with the grid and the brute form (which has a host form only), alternating within
    each repetition; both upload the same points.  `grid_beats_brute` is the one condition DESIGN.md holds the feature to.
  * with scipy importable: a greedy pass over a cKDTree on the CPU in the same order (for the record; its flags are compared).

No time is asserted.

  python3 tools/measure_poisson.py [--reps N] [--out profiles/poisson_measure.json] [--only NAME] [--n N] [--dragon TRIS]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402


def wall(reps, routes):
    """routes: name -> blocking call.  Medians and quartiles in ms on the host's clock, the routes alternating within each repetition."""
    for _ in range(3):
        for call in routes.values():
            call()
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            t[k].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for k, v in t.items():
        q1, med, q3 = np.percentile(v, [25, 50, 75])
        out[k] = {"median_ms": round(float(med), 4), "q1_ms": round(float(q1), 4), "q3_ms": round(float(q3), 4)}
    return out


def kdtree_greedy(points, min_dist2, seed):
    """The sequential pass with scipy's cKDTree for the neighbours (float64 distances: a candidate list, filtered by the f32 test)."""
    from scipy.spatial import cKDTree

    import poisson_ref as pref

    t0 = time.perf_counter()
    n = len(points)
    tree = cKDTree(points.astype(np.float64))
    r = math.sqrt(float(min_dist2)) * (1 + 1e-6)
    keep = np.zeros(n, bool)
    m = np.float32(min_dist2)
    for i in np.argsort(pref.keys(n, seed), kind="stable"):
        nb = np.asarray(tree.query_ball_point(points[i].astype(np.float64), r), np.int64)
        nb = nb[keep[nb]]
        if len(nb):
            d = points[i][None, :] - points[nb]
            if (((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < m).any():
                continue
        keep[i] = True
    return keep, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poisson_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--brute-n", type=int, default=65536)
    ap.add_argument("--dragon", type=int, default=800_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_poisson.py needs a GPU: a time taken elsewhere says nothing")
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    pkg = entry.load_package()
    rows = []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(a.dragon))
        sc = pkg.Scene(sd, device=0)
        area = sc.triangle_areas()[1]
        for n, brute in ((a.n, False), (a.brute_n, True)):
            pts = sc.sample_surface_tensor(n, seed=1, strata=n)["point"].contiguous()
            torch.cuda.synchronize()
            host = pts.cpu().numpy()
            mask = torch.empty((n,), dtype=torch.bool, device="cuda")
            ws = torch.empty((sc.poisson_disk_workspace(n),), dtype=torch.uint8, device="cuda")
            for k in (8, 64):
                m = float(np.float32(k * area / (math.pi * n)))
                row = {"scene": name, "triangles": int(sd.ntris), "candidates": n, "aimed_conflicts": k, "min_dist2": m}
                if not brute:
                    row.update(wall(a.reps, {"device_form": lambda: sc.poisson_disk_tensor(pts, m, seed=1, out=mask, workspace=ws)}))
                    flags = mask.cpu().numpy()
                else:
                    got = {}
                    t = wall(a.reps, {"grid_host_form": lambda: got.__setitem__("grid", sc.poisson_disk(host, m, seed=1)),
                                      "brute_host_form": lambda: got.__setitem__("brute", sc.poisson_disk_brute(host, m, seed=1))})
                    flags = got["grid"]
                    row.update(t)
                    row["same_flags"] = bool(np.array_equal(got["grid"], got["brute"]))
                    row["brute_over_grid"] = round(t["brute_host_form"]["median_ms"] / t["grid_host_form"]["median_ms"], 2)
                    row["grid_beats_brute"] = t["grid_host_form"]["median_ms"] < t["brute_host_form"]["median_ms"]
                    if have_scipy:
                        keep, ms = kdtree_greedy(host, m, 1)
                        row["ckdtree_greedy_cpu_ms"] = round(ms, 1)
                        row["ckdtree_same_flags"] = bool(np.array_equal(keep, flags))
                work = [sc.debug_poisson_work(host, m, seed=1) for _ in range(5)]
                row.update({"kept": int(flags.sum()), "rounds": work[0]["rounds"],
                            "pair_tests_per_candidate": round(work[0]["pair_tests"] / n, 2),
                            "buckets_used": work[0]["buckets_used"], "buckets": work[0]["buckets"],
                            "counted_build_ms": round(float(np.median([w["build_ns"] for w in work])) / 1e6, 4),
                            "counted_rounds_ms": round(float(np.median([w["rounds_ns"] for w in work])) / 1e6, 4)})
                rows.append(row)
                print(json.dumps(row), flush=True)
            del pts, mask, ws
            torch.cuda.empty_cache()
        sc.close()
    doc = {"device": torch.cuda.get_device_name(0), "sources": pkg.source_hash(), "reps": a.reps, "scipy": have_scipy,
           "timing": "host clock around the blocking call, ms, after a device synchronisation; routes of a row alternate within each repetition",
           "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

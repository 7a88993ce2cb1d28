"""The bitwise-reproducible form of the table adjoint (reproducible=True of Scene.surface_views_grad_tensor and
interpolate_hits_grad_tensor) on the rows of profiles/surface_grad_measure.json, against the two things a caller
has otherwise.  Device time between HIP events on the stream the work runs on, every shape warmed first, the routes taken in turn
(rotated from repetition to repetition); per route the median and the quartiles.

Workloads: (a) Cornell 1920 x 1080, frame form; (b) the 800 K dragon stand-in 1920 x 1080, frame form; (c) the same dragon frame's rays
as a list of 2 073 600 rays, list form.  Channels C = 3, 8, 16, 32, 64 (--channels for others), seeded random gradients, a table that is
accumulated into again and again.

Routes:
  repro                the reproducible entry: clear, max pass, add pass, finalise; its workspace (12 bytes per table element) comes
                       from torch's caching allocator inside the timed region, as a caller's would
  float                the float-atomic entry of the same library (surface_kernels.hip), which this form leaves unchanged
  torch_deterministic  three index_add_ of bary[:, k:k+1] * grad_out by tri[prim_id][:, k] under
                       torch.use_deterministic_algorithms(True): the only reproducible route a caller had; the barycentrics and the
                       gathered rows are computed before the clock starts

A call of the torch route takes seconds where the others take a millisecond or less; --torch-reps sets its repetitions apart (each
route's count is written next to its median), and --routes leaves routes out (ratios to a route left out are not written).

  python3 tools/measure_surface_grad_repro.py [--reps N] [--torch-reps N] [--routes repro,float,torch_deterministic] [--out FILE.json]
                                              [--only NAME] [--channels 3,8,16,32,64]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402

W, H = 1920, 1080
WORKLOADS = [("cornell_1080p_frame", "cornell", "frame"), ("dragon800k_1080p_frame", "dragon", "frame"), ("dragon800k_2m_list", "dragon", "list")]


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": float(med), "q1_ms": float(q1), "q3_ms": float(q3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int)
    ap.add_argument("--routes", default="repro,float,torch_deterministic")
    ap.add_argument("--out")
    ap.add_argument("--only")
    ap.add_argument("--channels", default="3,8,16,32,64")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_surface_grad_repro.py needs a GPU: a time taken elsewhere says nothing")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    channels = tuple(int(c) for c in a.channels.split(","))
    chosen = a.routes.split(",")
    if "repro" not in chosen or any(r not in ("repro", "float", "torch_deterministic") for r in chosen):
        raise SystemExit("--routes: repro, and any of float, torch_deterministic")
    reps = {r: a.torch_reps if r == "torch_deterministic" and a.torch_reps else a.reps for r in chosen}
    pkg = entry.load_package()
    os.environ.pop("CGRT_SURFACE_GRAD_MAP", None)
    results = {"reps": a.reps, "source_hash": pkg.source_hash(), "W": W, "H": H, "workloads": {}}
    scenes = {}
    for name, which, form in WORKLOADS:
        if a.only and a.only not in name:
            continue
        if which not in scenes:
            sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz")) if which == "cornell"
                  else pkg.scenes.make_dragon(800_000))
            scenes[which] = (sd, pkg.Scene(sd, device=0))
        sd, sc = scenes[which]
        cam = pkg.scenes.default_camera(W, H)
        n = W * H
        ntris, nverts = sd.ntris, len(sd.pos_nrm)
        tri = torch.from_numpy(np.asarray(sd.tri, np.int64).reshape(-1, 3)).cuda()
        hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        sc.trace_views_device(cam[None], W, H, hits.data_ptr())
        torch.cuda.synchronize()
        depth = hits[:, 0].view(torch.float32).reshape(1, H, W).contiguous()
        prim = hits[:, 1].reshape(1, H, W).contiguous()
        rays = torch.from_numpy(sc.generate_rays(cam, W, H).view(np.float32).reshape(-1, 7).copy()).cuda() if form == "list" else None
        flat = prim.reshape(-1)
        on_tri = (flat >= 0) & (flat < ntris)
        rows = tri[flat.clamp(0, max(ntris - 1, 0)).long()]
        bary = (sc.surface_views_tensor(cam, W, H, depth, prim)["bary"] if form == "frame" else sc.hit_barycentrics_tensor(rays, hits)).reshape(-1, 3)
        torch.cuda.synchronize()
        changes = int((flat[1:] != flat[:-1]).sum().item()) + 1
        res = {"triangle_hits": int(on_tri.sum().item()), "items": n, "nverts": nverts, "mean_run_of_one_prim_id": n / changes, "channels": {}}
        for C in channels:
            g = torch.from_numpy(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32)).cuda()
            g_call = g.reshape(1, H, W, C) if form == "frame" else g
            tables = {r: torch.zeros((nverts, C), dtype=torch.float32, device="cuda") for r in ("repro", "float", "torch_deterministic")}

            def grad(route):
                if form == "frame":
                    sc.surface_views_grad_tensor(cam, W, H, depth, prim, g_call, grad_attr=tables[route], reproducible=route == "repro")
                else:
                    sc.interpolate_hits_grad_tensor(rays, hits, g_call, grad_attr=tables[route], reproducible=route == "repro")

            def composed():
                torch.use_deterministic_algorithms(True)
                try:
                    for k in range(3):
                        tables["torch_deterministic"].index_add_(0, rows[:, k], bary[:, k : k + 1] * g)
                finally:
                    torch.use_deterministic_algorithms(False)

            routes = {"repro": lambda: grad("repro"), "float": lambda: grad("float"), "torch_deterministic": composed}
            order = [r for r in routes if r in chosen]
            for k in range(3):  # warm: code objects, the lookup table, torch's allocator (the torch route, seconds a call: once)
                for r in order:
                    if k == 0 or r != "torch_deterministic":
                        routes[r]()
            torch.cuda.synchronize()
            # one call of each into a fresh table: the reproducible form twice gives the same bytes, and agrees with the others to rounding
            for t in tables.values():
                t.zero_()
            for r in order:
                routes[r]()
            first = tables["repro"].clone()
            tables["repro"].zero_()
            routes["repro"]()
            same = bool(torch.equal(first.view(torch.int32), tables["repro"].view(torch.int32)))
            scale = max(float(tables["repro"].abs().max().item()), 1e-30)
            agree = {r: float((tables["repro"] - tables[r]).abs().max().item()) / scale for r in order if r != "repro"}
            for t in tables.values():
                t.zero_()
            events = {r: [] for r in order}
            for i in range(max(reps.values())):
                k = i % len(order)
                for r in order[k:] + order[:k]:
                    if i >= reps[r]:
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    routes[r]()
                    e1.record()
                    events[r].append((e0, e1))
                torch.cuda.synchronize()
            stats = {r: quartiles([e0.elapsed_time(e1) for e0, e1 in v]) for r, v in events.items()}
            contributions = res["triangle_hits"] * 3 * C
            ms = stats["repro"]["median_ms"]
            res["channels"][str(C)] = {
                "routes": stats,
                **{f"repro_over_{r}": ms / stats[r]["median_ms"] for r in order if r != "repro"},
                "second_call_same_bytes": same,
                "max_abs_difference_of_repro_over_max_abs": agree,
                "bytes_model": {"contributions_uncombined": contributions, "max_pass_atomic_bytes": 4 * contributions,
                                "add_pass_atomic_bytes": 8 * contributions, "workspace_bytes": 12 * nverts * C,
                                "cleared_bytes": 12 * nverts * C, "finalise_read_bytes_at_least": 4 * nverts * C},
                "atomic_TBps_if_all_time_were_the_two_passes": 12 * contributions / (ms * 1e-3) / 1e12}
            print(name, "C", C, json.dumps({r: round(s["median_ms"], 4) for r, s in stats.items()}), "same bytes twice:", same,
                  "difference / max:", agree, flush=True)
        results["workloads"][name] = res
    for _, sc in scenes.values():
        sc.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()

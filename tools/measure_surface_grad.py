"""Gradients of the surface attributes back to the per-vertex table (Scene.surface_views_grad_tensor, interpolate_hits_grad_tensor;
DESIGN.md section 5.23) against what a caller would compose in torch, and against the forward call for scale.  Device time between HIP
events on the stream the work runs on, every shape warmed first, the routes taken in turn (rotated from repetition to repetition); per
route the median and the quartiles.

Workloads: (a) Cornell 1920 x 1080, frame form; (b) the 800 K dragon stand-in 1920 x 1080, frame form; (c) the same dragon frame's rays
as a list of 2 073 600 rays, list form.  Channels C = 3 and C = 32 (--channels for others), seeded random gradients, a zeroed table that
is accumulated into again and again.

Routes:
  grad             the gradient call as shipped (surface_kernels.hip surface_grad_policy)
  grad:element     the same call with lanes walking the wave's contiguous 64 x C run            (CGRT_SURFACE_GRAD_MAP=element)
  grad:item        lane = item, consecutive lanes of one prim_id summed inside the wave first   (CGRT_SURFACE_GRAD_MAP=item)
  grad:item_plain  lane = item, every lane adds                                                 (CGRT_SURFACE_GRAD_MAP=item_plain)
  torch            the composition: three index_add_ of bary[:, k:k+1] * grad_out by tri[prim_id][:, k]; the barycentrics and the
                   gathered rows are computed before the clock starts
  forward          the forward call (the interpolated attribute only), for scale

  python3 tools/measure_surface_grad.py [--reps N] [--out FILE.json] [--only NAME] [--channels 3,32]
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
KNOB = "CGRT_SURFACE_GRAD_MAP"
GUIDE_ATOMIC_TBPS = 1.3  # the chip-wide rate of no-return f32 atomic adds in their best shape, as published for this chip


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, np.float64), [25, 50, 75])
    return {"median_ms": float(med), "q1_ms": float(q1), "q3_ms": float(q3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    ap.add_argument("--only")
    ap.add_argument("--channels", default="3,32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_surface_grad.py needs a GPU: a time taken elsewhere says nothing")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    channels = tuple(int(c) for c in a.channels.split(","))
    pkg = entry.load_package()
    os.environ.pop(KNOB, None)
    results = {"reps": a.reps, "source_hash": pkg.source_hash(), "W": W, "H": H, "guide_atomic_TBps": GUIDE_ATOMIC_TBPS, "workloads": {}}
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
        res = {"triangle_hits": int(on_tri.sum().item()), "items": n, "mean_run_of_one_prim_id": n / changes, "channels": {}}
        for C in channels:
            g = torch.from_numpy(np.random.default_rng(C).standard_normal((n, C)).astype(np.float32)).cuda()
            g_call = g.reshape(1, H, W, C) if form == "frame" else g
            attr = torch.from_numpy(np.random.default_rng(C + 1).standard_normal((nverts, C)).astype(np.float32)).cuda()
            table = torch.zeros((nverts, C), dtype=torch.float32, device="cuda")
            table_t = torch.zeros_like(table)
            o_a = torch.empty((1, H, W, C) if form == "frame" else (n, C), dtype=torch.float32, device="cuda")

            def grad(knob=None):
                if knob is None:
                    os.environ.pop(KNOB, None)
                else:
                    os.environ[KNOB] = knob
                if form == "frame":
                    sc.surface_views_grad_tensor(cam, W, H, depth, prim, g_call, grad_attr=table)
                else:
                    sc.interpolate_hits_grad_tensor(rays, hits, g_call, grad_attr=table)
                os.environ.pop(KNOB, None)

            def composed():
                for k in range(3):
                    table_t.index_add_(0, rows[:, k], bary[:, k : k + 1] * g)

            def forward():
                if form == "frame":
                    sc.surface_views_tensor(cam, W, H, depth, prim, attr=attr, want_bary=False, out={"attr": o_a})
                else:
                    sc.interpolate_hits_tensor(rays, hits, attr, out=o_a)

            routes = {"grad": grad, "grad:element": lambda: grad("element"), "grad:item": lambda: grad("item"),
                      "grad:item_plain": lambda: grad("item_plain"), "torch": composed, "forward": forward}
            order = list(routes)
            for _ in range(3):  # warm: code objects, the lookup table, torch's allocator
                for r in order:
                    routes[r]()
            torch.cuda.synchronize()
            # one call of each into a fresh table: the two routes agree to rounding (not bit for bit: the orders differ)
            table.zero_()
            table_t.zero_()
            grad()
            composed()
            scale = float(table_t.abs().max().item())
            agree = float((table - table_t).abs().max().item()) / max(scale, 1e-30)
            table.zero_()
            table_t.zero_()
            events = {r: [] for r in order}
            for i in range(a.reps):
                k = i % len(order)
                for r in order[k:] + order[:k]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    routes[r]()
                    e1.record()
                    events[r].append((e0, e1))
                torch.cuda.synchronize()
            stats = {r: quartiles([e0.elapsed_time(e1) for e0, e1 in v]) for r, v in events.items()}
            added = res["triangle_hits"] * 3 * C * 4
            res["channels"][str(C)] = {
                "routes": stats, "max_abs_difference_to_torch_over_max_abs": agree,
                "added_bytes_uncombined": added,
                "added_TBps": {r: added / (stats[r]["median_ms"] * 1e-3) / 1e12 for r in order if r.startswith("grad")},
                "bytes_model": {"read_per_item": (8 if form == "frame" else 44) + 4 * C, "read_per_triangle_hit": 16 + 48,
                                "added_per_triangle_hit": 12 * C}}
            print(name, "C", C, json.dumps({r: round(s["median_ms"], 4) for r, s in stats.items()}), "difference to torch / max:", agree, flush=True)
        results["workloads"][name] = res
    for _, sc in scenes.values():
        sc.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()

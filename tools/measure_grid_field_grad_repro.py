"""The bitwise-reproducible form of the sampler's adjoint (Scene.sample_grid_grad_device(..., reproducible=True))
against the float entry of the same library (section 5.35) and against the backward of torch.nn.functional.grid_sample(align_corners=True)
with respect to its input, plain and under torch.use_deterministic_algorithms(True), on the same device.

The rows are those of tools/measure_grid_field_grad.py, as they are: dodge (tests/golden) and the 800 K dragon stand-in; per scene and per
side (128, 256) the grid over the scene box grown by 25 %, its values made by sdf_grid_tensor; two sets of 1 048 576 points, `uniform`
in the grid's box and `surface`, the hit points of march_grid_tensor from 1024 x 1024 camera rays (the contended case).
Routes of a row:
  repro_value / repro_gradient / repro_both   the reproducible entry with grad_value only, grad_gradient only, both, into a preallocated
                                              volume, its workspace (12 bytes per grid element) preallocated too
  float_value / float_gradient / float_both   the float-atomic entry, the same inputs
  torch                                       the backward of grid_sample's trilinear value with respect to the volume
  torch_deterministic                         the same under torch.use_deterministic_algorithms(True), if torch offers one: if it raises,
                                              the message is recorded and the route is left out
Everything is preallocated; every route is warmed first and timed between HIP events on the current stream; the routes ALTERNATE within
each repetition.  Per row the tool also checks that a second reproducible call gives the first one's bytes and reports the largest
difference from the float entry relative to the largest element.  No time is asserted.

The four passes (clear, max, add, finalise) are kernel times and come from a trace, in a run of its own:
  python3 tools/measure_grid_field_grad_repro.py [--reps N] [--out profiles/grid_field_grad_repro_measure.json] [--only NAME] [--sides 128,256]
  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 tools/measure_grid_field_grad_repro.py --passes ORDER.json [...]
  python3 tools/measure_grid_field_grad_repro.py --merge-passes DIR --passes ORDER.json [--out ...]
--passes runs, per row, 3 + reps reproducible calls with both grads and nothing else of this library, and writes the rows' order;
--merge-passes reads every *kernel_trace.csv under DIR, takes the dispatches of each call in time order (the clear is the fill kernels right
before the max pass) and writes the medians of the timed calls, in microseconds, into the rows of --out as
"passes_us"; a pass the trace does not show is written as "not measured".
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WARM = 3


def merge_passes(trace_dir, order_file, out):
    with open(order_file) as f:
        order = json.load(f)
    disp = []
    for fn in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(fn, newline="") as f:
            for r in csv.DictReader(f):
                disp.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    if not disp:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    disp.sort()
    calls = []  # per reproducible call: [clear, max, add, finalise] in ns, None where the trace does not show it
    k = 0
    while k < len(disp):
        name = disp[k][2]
        if "k_sample_grid_grad_repro" in name and "finalise" not in name:
            if k + 2 >= len(disp) or "k_sample_grid_grad_repro" not in disp[k + 1][2] or "finalise" not in disp[k + 2][2]:
                sys.exit(f"dispatch {k}: the max pass is not followed by the add pass and the finalise")
            clear, j = None, k - 1
            while j >= 0 and "fill" in disp[j][2].lower():  # (a memset may be more than one fill kernel)
                clear = (clear or 0) + disp[j][1] - disp[j][0]
                j -= 1
            calls.append([clear] + [disp[j][1] - disp[j][0] for j in (k, k + 1, k + 2)])
            k += 3
        else:
            k += 1
    per_row = WARM + order["reps"]
    if len(calls) != per_row * len(order["rows"]):
        sys.exit(f"{len(calls)} reproducible calls in the trace, {per_row * len(order['rows'])} expected")
    with open(out) as f:
        doc = json.load(f)
    for i, key in enumerate(order["rows"]):
        timed = calls[i * per_row + WARM:(i + 1) * per_row]
        med = {}
        for j, p in enumerate(("clear", "max", "add", "finalise")):
            vals = [c[j] for c in timed if c[j] is not None]
            med[p] = round(float(np.median(vals)) / 1e3, 1) if len(vals) == len(timed) else "not measured"
        for row in doc["rows"]:
            if [row["scene"], row["side"], row["set"]] == key:
                row["passes_us"] = med
        print(key, med, flush=True)
    doc["passes"] = ("kernel times of one rocprofv3 --kernel-trace run of this tool with --passes (both grads), medians of the timed calls, "
                     "microseconds; the clear is the fill kernel of hipMemsetAsync")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_field_grad_repro_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--sides", default="128,256")
    ap.add_argument("--rays-side", type=int, default=1024)
    ap.add_argument("--passes", metavar="ORDER.json", help="the reduced run for a kernel trace; writes the rows' order there")
    ap.add_argument("--merge-passes", metavar="TRACE_DIR")
    a = ap.parse_args()
    if a.merge_passes:
        if not a.passes:
            sys.exit("--merge-passes needs --passes ORDER.json, the file the traced run wrote")
        return merge_passes(a.merge_passes, a.passes, a.out)
    import torch  # (first: torch's HIP runtime is the one libcgrt.so binds to)

    import __graft_entry__ as entry
    import closest_ref as cr
    import grid_field_grad_ref as aref
    from measure_grid_field import camera_rays
    from measure_sdf import timed

    if not torch.cuda.is_available():
        raise SystemExit("measure_grid_field_grad_repro.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    Fn = torch.nn.functional
    rows, order = [], []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        lo, hi = cr.scene_box(sd)
        ext = np.maximum(hi - lo, 1e-3)
        rays_h = camera_rays(lo, hi, a.rays_side)
        n = len(rays_h)
        rays = torch.from_numpy(rays_h).cuda()
        st = torch.cuda.current_stream().cuda_stream
        rng = np.random.default_rng(17)
        gv_h, gg_h = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        gv, gg = torch.from_numpy(gv_h).cuda(), torch.from_numpy(gg_h).cuda()
        for side in (int(x) for x in a.sides.split(",")):
            origin, spacing, dims = (lo - 0.25 * ext).astype(np.float32), (1.5 * ext / (side - 1)).astype(np.float32), (side,) * 3
            values = sc.sdf_grid_tensor(origin, spacing, dims, want="sdf")
            extent = float(ext.max())
            rec = sc.march_grid_tensor(values, origin, spacing, rays, iso=0.0, relax=1.0, min_step=1e-4 * extent, hit_eps=1e-4 * extent,
                                       max_steps=256, refine=8)
            hit = (rec["status"] == 1).cpu().numpy()
            if not hit.any():
                raise SystemExit(f"{name} {side}: no ray hit the level")
            t_h = rec["t"].cpu().numpy()
            surf = (rays_h[hit, 0:3] + t_h[hit, None] * rays_h[hit, 3:6]).astype(np.float32)
            surf = surf[np.random.default_rng(side).integers(0, len(surf), n)] if len(surf) < n else surf[:n]
            sets = {"uniform": (origin + np.random.default_rng(side).uniform(0, 1, size=(n, 3)) * (1.5 * ext)).astype(np.float32),
                    "surface": np.ascontiguousarray(surf)}
            o_t, s_t = torch.from_numpy(origin).cuda(), torch.from_numpy(spacing * (side - 1)).cuda()
            out = torch.zeros(dims[::-1], dtype=torch.float32, device="cuda")
            ws_bytes = sc.sample_grid_grad_repro_workspace(origin, spacing, dims)
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
            assert ws.data_ptr() % 8 == 0
            for set_name, pts_h in sets.items():
                pts = torch.from_numpy(pts_h).cuda()

                def call(v, g, repro, into=out):
                    kw = dict(reproducible=True, d_workspace_ptr=ws.data_ptr(), workspace_bytes=ws_bytes) if repro else {}
                    return lambda: sc.sample_grid_grad_device(origin, spacing, dims, pts.data_ptr(), n, v.data_ptr() if v is not None else 0,
                                                              g.data_ptr() if g is not None else 0, into.data_ptr(), stream=st, **kw)

                if a.passes:
                    for _ in range(WARM + a.reps):
                        call(gv, gg, True)()
                    torch.cuda.synchronize()
                    order.append([name, side, set_name])
                    print("traced", name, side, set_name, flush=True)
                    continue
                vol = torch.zeros_like(values)[None, None].requires_grad_(True)
                coords = ((pts - o_t) / s_t * 2 - 1)[None, None, None]
                sampled = Fn.grid_sample(vol, coords, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, 0, 0]
                routes = {}
                for key, (v, g) in (("value", (gv, None)), ("gradient", (None, gg)), ("both", (gv, gg))):
                    routes["repro_" + key] = call(v, g, True)
                    routes["float_" + key] = call(v, g, False)
                routes["torch"] = lambda: torch.autograd.grad(sampled, vol, gv, retain_graph=True)
                torch_det = None
                try:  # does torch offer a deterministic backward here?
                    torch.use_deterministic_algorithms(True)
                    torch.autograd.grad(sampled, vol, gv, retain_graph=True)
                    torch.cuda.synchronize()

                    def det():
                        torch.use_deterministic_algorithms(True)
                        try:
                            return torch.autograd.grad(sampled, vol, gv, retain_graph=True)
                        finally:
                            torch.use_deterministic_algorithms(False)

                    routes["torch_deterministic"] = det
                except RuntimeError as e:
                    torch_det = "raises: " + str(e).split("\n")[0][:300]
                finally:
                    torch.use_deterministic_algorithms(False)
                t = timed(a.reps, routes)
                # the bytes: two reproducible calls from zero agree; the float entry differs in the last bits
                one, two, flt = (torch.zeros_like(out) for _ in range(3))
                call(gv, gg, True, one)(), call(gv, gg, True, two)(), call(gv, gg, False, flt)()
                torch.cuda.synchronize()
                same = bool((one.view(torch.int32) == two.view(torch.int32)).all())
                rel = float((one.double() - flt.double()).abs().max() / one.double().abs().max())
                inside, index, _ = aref.contributions(origin, spacing, dims, pts_h, gv_h, None)
                row = {"scene": name, "triangles": int(sd.ntris), "side": side, "set": set_name, "n": n,
                       "distinct_cells": int(len(np.unique(index[inside, 0]))), "workspace_MB": round(ws_bytes / 1e6, 1),
                       "second_call_same_bytes": same, "max_abs_diff_from_float_over_max_abs": rel, **t}
                if torch_det:
                    row["torch_deterministic"] = torch_det
                for key in ("value", "gradient", "both"):
                    med = t["repro_" + key]["median_ms"]
                    row[f"repro_{key}_over_float"] = round(med / t["float_" + key]["median_ms"], 3)
                    row[f"spread_repro_{key}"] = round((t["repro_" + key]["q3_ms"] - t["repro_" + key]["q1_ms"]) / med, 4)
                row["repro_value_over_torch"] = round(t["repro_value"]["median_ms"] / t["torch"]["median_ms"], 3)
                if "torch_deterministic" in t:
                    row["repro_value_over_torch_deterministic"] = round(t["repro_value"]["median_ms"] / t["torch_deterministic"]["median_ms"], 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
        sc.close()
    if a.passes:
        with open(a.passes, "w") as f:
            json.dump({"reps": a.reps, "rows": order}, f)
        print("wrote", a.passes)
        return
    doc = {"device": torch.cuda.get_device_name(0), "sources": pkg.source_hash(), "reps": a.reps,
           "timing": "device time between HIP events, ms; the routes of a row alternate within each repetition",
           "passes": "not measured", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

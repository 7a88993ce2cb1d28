"""Surface sampling (Scene.sample_surface_tensor): the fused kernel against the composition a user writes in torch
on the same device from the same thresholds -- torch-made random words, torch.searchsorted, the vertex-index gather, three position
gathers and the mix (with a table: three more gathers and a second mix).  The composition is the yardstick, not a reference: its random
numbers are torch's, so the points differ; what is compared is the time to produce n area-weighted points (and rows).

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Per scene 1 048 576 and 16 777 216 samples, independent and stratified,
without a table and with a C = 3 table (the vertex positions).

The fused call writes into preallocated tensors; the composition allocates its intermediates from torch's caching allocator, as it would
in use.  Every route is warmed first and timed between HIP events on the current stream; the two routes of a row ALTERNATE within each
repetition.  A row holds the median and quartiles of both, `spread` = (q3 - q1) / median of the fused route, and the factor composition /
fused.  No time is asserted.

  python3 tools/measure_sampling.py [--reps N] [--out profiles/sampling_measure.json] [--only NAME] [--n N ...] [--dragon TRIS]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402
from measure_sdf import timed  # noqa: E402


def composition(T, tri, pos, attr, n, strata):
    """n area-weighted points (and rows) in plain torch: T the first `last` thresholds (int64), tri (ntris, 3) int64, pos (nverts, 3)."""
    x = torch.randint(0, 1 << 32, (n,), dtype=torch.int64, device=T.device)
    if strata:
        x = ((torch.arange(n, dtype=torch.int64, device=T.device) << 32) | x) // strata
    prim = torch.searchsorted(T, x, right=True)
    u = torch.rand((n, 2), device=T.device)
    u = torch.where((u.sum(1) > 1.0)[:, None], 1.0 - u, u)
    b0, b1, b2 = (1.0 - u[:, 0] - u[:, 1])[:, None], u[:, 0:1], u[:, 1:2]
    idx = tri[prim]
    i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
    point = (b0 * pos[i0] + b1 * pos[i1]) + b2 * pos[i2]
    rows = None if attr is None else (b0 * attr[i0] + b1 * attr[i1]) + b2 * attr[i2]
    return point, prim, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_measure.json"))
    ap.add_argument("--only")
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 20, 1 << 24])
    ap.add_argument("--dragon", type=int, default=800_000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_sampling.py needs a GPU: a time taken elsewhere says nothing")
    pkg = entry.load_package()
    rows = []
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(a.dragon))
        sc = pkg.Scene(sd, device=0)
        before = sc.device_bytes()
        tab = sc.debug_sample_table()
        T = torch.from_numpy(tab["thresholds"][: tab["last"]].astype(np.int64)).cuda()
        tri = torch.from_numpy(np.asarray(sd.tri, np.int64).reshape(-1, 3)).cuda()
        pos = torch.from_numpy(np.ascontiguousarray(np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3])).cuda()
        for n in a.n:
            out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            out_rows = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            for stratified in (False, True):
                for table in (False, True):
                    strata = n if stratified else 0
                    attr = pos if table else None
                    routes = {
                        "fused": lambda: sc.sample_surface_tensor(n, seed=1, strata=strata, attr=attr, out=out, out_attr=out_rows if table else None),
                        "torch_composition": lambda: composition(T, tri, pos, attr, n, strata),
                    }
                    t = timed(a.reps, routes)
                    _, prim, _ = composition(T, tri, pos, attr, n, strata)
                    torch.cuda.synchronize()
                    f, c = t["fused"], t["torch_composition"]
                    row = {"scene": name, "triangles": int(sd.ntris), "samples": n, "stratified": stratified, "table_channels": 3 if table else 0, **t,
                           "spread": round((f["q3_ms"] - f["q1_ms"]) / f["median_ms"], 4),
                           "fused_msamples_per_s": round(n / f["median_ms"] / 1e3, 1),
                           "composition_over_fused": round(c["median_ms"] / f["median_ms"], 3),
                           "fused_at_least_as_fast": f["median_ms"] <= c["median_ms"],
                           "composition_prims_in_range": bool(int(prim.max().item()) <= tab["last"])}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
            del out, out_rows
            torch.cuda.empty_cache()
        rows.append({"scene": name, "sampling_device_bytes": int(sc.device_bytes() - before), "scene_device_bytes": int(before)})
        sc.close()
    doc = {"device": torch.cuda.get_device_name(0), "sources": pkg.source_hash(), "reps": a.reps,
           "timing": "device time between HIP events, ms; the two routes of a row alternate within each repetition",
           "lds_top_variant": "not tried", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Times the visibility queries on the device, HIP events on one torch stream, after warm-up:

  1. cgrt_occluded_device against cgrt_intersect_batch_device on the SAME lists: the level-0 point-light shadow rays of the Cornell
     800x800 and the 800 K dragon 1080p frames (t = FLT_MAX, as spawned), and 1 M random segments (finite t) about the dragon;
  2. cgrt_in_shadow_device against what a caller does without it: spawn the shadow rays on the host, upload them,
     cgrt_intersect_batch_device, download the hits and take the verdict on the host -- for the dragon's 1080p hit points x 1 and x 4
     lights;
  3. cgrt_soft_lit_device on the Cornell 800x800 hit points x the spherical preset at 200 samples, any-hit against closest-hit.

Prints one JSON object (milliseconds, medians of --reps).  Usage: python tools/measure_visibility.py [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import occlfam  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def timed(torch, stream, fn, reps, warm=3):
    for _ in range(warm):
        fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def hit_points(sc, cam, W, H):
    hits, _ = sc.trace_primary(cam, W, H)
    rays = sc.generate_rays(cam, W, H).view(np.float32).reshape(-1, 7)
    m = hits["hit"] == 1
    return (rays[m, 0:3] + rays[m, 3:6] * hits["t"][m][:, None]).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    pkg = load_package()
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    res = {"reps": a.reps}

    def lists(sc, rays, tag):
        tr = torch.from_numpy(np.ascontiguousarray(rays, np.float32)).to(dev)
        n = len(rays)
        hb = torch.empty(n, dtype=torch.uint8, device=dev)
        hh = torch.empty((n, 4), dtype=torch.int32, device=dev)
        s = st.cuda_stream
        any_ms = timed(torch, st, lambda: sc.occluded_device(tr.data_ptr(), n, hb.data_ptr(), stream=s), a.reps)
        cl_ms = timed(torch, st, lambda: sc.intersect_device(tr.data_ptr(), n, hh.data_ptr(), stream=s), a.reps)
        st.synchronize()
        same = bool(torch.equal(hb.to(torch.int32), hh[:, 3]))
        res[tag] = dict(rays=n, occluded_ms=any_ms, intersect_ms=cl_ms, ratio=cl_ms / any_ms, flags_equal=same)

    sd_c = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))
    sd_d = pkg.scenes.make_dragon(800_000)
    sc_c, sc_d = pkg.Scene(sd_c), pkg.Scene(sd_d)
    pc = hit_points(sc_c, pkg.scenes.default_camera(800, 800), 800, 800)
    pd = hit_points(sc_d, pkg.scenes.default_camera(1920, 1080), 1920, 1080)
    lc, ld = np.asarray(sd_c.point_lights, np.float32).reshape(-1, 6), np.asarray(sd_d.point_lights, np.float32).reshape(-1, 6)

    # 1. the same lists both ways
    lists(sc_c, occlfam.spawn(pc, lc[:, 0:3])[0], "cornell_800_shadow_rays")
    lists(sc_d, occlfam.spawn(pd, ld[:, 0:3])[0], "dragon_1080p_shadow_rays")
    rng = np.random.default_rng(1)
    p = np.asarray(sd_d.pos_nrm, np.float32)[:, :3]
    lo, hi = p.min(0), p.max(0)
    o = (lo + rng.uniform(-0.2, 1.2, (1 << 20, 3)) * (hi - lo)).astype(np.float32)
    e = (lo + rng.uniform(-0.2, 1.2, (1 << 20, 3)) * (hi - lo)).astype(np.float32)
    seg = np.concatenate([o, occlfam.normalize(e - o), occlfam.length(e - o)[:, None]], 1).astype(np.float32)
    lists(sc_d, seg, "dragon_1M_random_segments")

    # 2. point-light query against spawn -> upload -> intersect -> verdict
    for k in (1, 4):
        L = np.concatenate([ld, (ld + np.float32([0.7, 0.3, -0.5, 0, 0, 0]) * np.arange(1, 4, dtype=np.float32)[:, None])])[:k] if k > 1 else ld[:1]
        L = np.ascontiguousarray(L, np.float32)
        tp = torch.from_numpy(pd).to(dev)
        out = torch.empty((len(pd), k), dtype=torch.uint8, device=dev)
        q_ms = timed(torch, st, lambda: sc_d.in_shadow_device(tp.data_ptr(), len(pd), out.data_ptr(), stream=st.cuda_stream, lights=L), a.reps)
        q_wall = wall(lambda: sc_d.in_shadow_device(tp.data_ptr(), len(pd), out.data_ptr(), stream=st.cuda_stream, lights=L), a.reps)
        hh = torch.empty((len(pd) * k, 4), dtype=torch.int32, device=dev)

        def manual():
            rays, dist = occlfam.spawn(pd, L[:, 0:3])
            tr = torch.from_numpy(rays).to(dev)
            sc_d.intersect_device(tr.data_ptr(), len(rays), hh.data_ptr(), stream=st.cuda_stream)
            st.synchronize()
            h = hh.cpu().numpy()
            return occlfam.verdict(h[:, 3], h[:, 0].view(np.float32), dist)

        m_wall = wall(manual, max(3, a.reps // 4))
        st.synchronize()
        same = bool(np.array_equal(out.cpu().numpy().reshape(-1).astype(bool), manual()))
        res[f"dragon_1080p_in_shadow_x{k}"] = dict(points=len(pd), lights=k, query_device_ms=q_ms, query_wall_ms=q_wall, manual_wall_ms=m_wall,
                                                  verdicts_equal=same)

    # 3. soft shadows: any-hit against closest-hit
    sl = pkg.scenes.CORNELL_SPHERICAL_LIGHTS  # the reference's CornellBoxSphericalLight preset
    units = pkg.unit_vector_table()
    tp = torch.from_numpy(pc).to(dev)
    lit = torch.empty((len(pc), len(sl)), dtype=torch.int32, device=dev)
    soft = {}
    for ch in (False, True):
        soft["closest_ms" if ch else "anyhit_ms"] = timed(
            torch, st, lambda: sc_c.soft_lit_device(tp.data_ptr(), len(pc), lit.data_ptr(), sl, units, samples=200, closest_hit=ch, stream=st.cuda_stream),
            max(3, a.reps // 2))
    res["cornell_800_soft_lit_200"] = dict(points=len(pc), samples=200, **soft, ratio=soft["closest_ms"] / soft["anyhit_ms"])
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()

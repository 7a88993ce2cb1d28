"""Crossing queries (Scene.count_crossings_tensor, list_crossings_tensor, first_crossings_tensor): count, full
list and first-4 against one closest-hit call on the same rays, and against the brute-force list.

Scenes: dodge (tests/golden) and the 800 K dragon stand-in.  Ray lists of 4 096, 65 536 and 1 048 576 rays of two families: the default
camera's frame (64 x 64, 256 x 256, 1024 x 1024) and interior rays (tests/crossings_ref.py random_rays: origins in the scene box grown by
25 %, random directions).

Routes, every shape warmed first, device time between HIP events on the current stream, median and quartiles over --reps calls:
  count     count_crossings_tensor into a preallocated tensor
  list      list_crossings_tensor: count, torch cumsum, the read-back of the total (a synchronisation), the allocation, the list
  first4    first_crossings_tensor(k = 4) into a preallocated tensor, with counts
  closest   intersect_device (cgrt_intersect_batch_device) on the same rays: the closest-hit walk the library already had
  brute     list_crossings_brute(k = 4): wall time of the host call (the library has no device form of the validation path; it carries
            the call's transfers); only where rays x triangles <= 2^34, 5 repetitions; its bytes are compared with first4's
  work      debug_crossing_work on 65 536 rays at most, evenly picked from the list (a counting launch, not timed)
No time is asserted anywhere.

  python3 tools/measure_crossings.py [--reps N] [--out profiles/crossings_bench.txt] [--only NAME]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (first: torch's HIP runtime is the one libcgrt.so binds to)

import __graft_entry__ as entry  # noqa: E402
import crossings_ref as xr  # noqa: E402

SIDES = (64, 256, 1024)
BRUTE_CAP = 1 << 34  # rays x triangles


def timed(reps, call):
    for _ in range(5):  # warm: the code object, torch's allocator, the caches
        call()
    torch.cuda.synchronize()
    events = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        events.append((e0, e1))
    torch.cuda.synchronize()
    q1, med, q3 = np.percentile([e0.elapsed_time(e1) for e0, e1 in events], [25, 50, 75])
    return float(med), float(q1), float(q3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossings_bench.txt"))
    ap.add_argument("--only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_crossings.py needs a GPU: a time taken elsewhere says nothing")
    if a.reps < 20:
        raise SystemExit("at least 20 repetitions")
    pkg = entry.load_package()
    orc = entry.load_oracle()
    lines = [f"crossing queries on {torch.cuda.get_device_name(0)}, sources {pkg.source_hash()}, {a.reps} repetitions per figure",
             "device time between HIP events in ms: median (q1 .. q3); brute: wall time of the host call, 5 repetitions", ""]
    fmt = lambda t: f"{t[0]:9.3f} ({t[1]:.3f} .. {t[2]:.3f})"  # noqa: E731
    for name in ("dodge", "dragon800k"):
        if a.only and a.only not in name:
            continue
        sd = (pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "dodge.npz")) if name == "dodge"
              else pkg.scenes.make_dragon(800_000))
        sc = pkg.Scene(sd, device=0)
        interior = xr.random_rays(sd, SIDES[-1] ** 2, 7)
        for fam in ("camera", "interior"):
            for side in SIDES:
                n = side * side
                rays = orc.generate_rays(pkg.scenes.default_camera(side, side), side, side) if fam == "camera" else interior[:n]
                rays = np.ascontiguousarray(rays, np.float32)
                d_rays = torch.from_numpy(rays).cuda()
                counts = torch.empty((n,), dtype=torch.int32, device="cuda")
                first = torch.empty((n, 4, 2), dtype=torch.float32, device="cuda")
                hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
                t_count = timed(a.reps, lambda: sc.count_crossings_tensor(d_rays, out=counts))
                t_list = timed(a.reps, lambda: sc.list_crossings_tensor(d_rays))
                t_first = timed(a.reps, lambda: sc.first_crossings_tensor(d_rays, 4, out=first))
                t_closest = timed(a.reps, lambda: sc.intersect_device(d_rays.data_ptr(), n, hits.data_ptr(),
                                                                      stream=torch.cuda.current_stream().cuda_stream))
                torch.cuda.synchronize()
                c = counts.cpu().numpy()
                m = min(n, 65536)
                nodes, tris = sc.debug_crossing_work(rays[:: n // m][:m])
                lines.append(f"{name} ({sd.ntris} triangles), {fam} rays, n = {n}: {c.mean():.2f} crossings per ray (largest {int(c.max())}); "
                             f"{nodes / m:.1f} node steps and {tris / m:.1f} triangles evaluated per ray")
                lines.append(f"  count   {fmt(t_count)}   {n / t_count[0] / 1e3:9.1f} M rays/s")
                lines.append(f"  list    {fmt(t_list)}   {n / t_list[0] / 1e3:9.1f} M rays/s")
                lines.append(f"  first4  {fmt(t_first)}   {n / t_first[0] / 1e3:9.1f} M rays/s")
                lines.append(f"  closest {fmt(t_closest)}   {n / t_closest[0] / 1e3:9.1f} M rays/s")
                if n * sd.ntris <= BRUTE_CAP:
                    want, _ = sc.list_crossings_brute(rays, k=4)  # (warms the call lane's buffers as well)
                    got = first.cpu().numpy().view(pkg.CROSSING_DTYPE).reshape(n, 4)
                    walls = []
                    for _ in range(5):
                        t0 = time.perf_counter()
                        sc.list_crossings_brute(rays, k=4)
                        walls.append((time.perf_counter() - t0) * 1e3)
                    q1, med, q3 = np.percentile(walls, [25, 50, 75])
                    lines.append(f"  brute   {fmt((med, q1, q3))}   bytes equal to first4: {got.tobytes() == want.tobytes()}")
                else:
                    lines.append("  brute   beyond 2^34 ray-triangle pairs: not run")
                print("\n".join(lines[-6:]), flush=True)
        sc.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

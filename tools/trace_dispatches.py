"""A fixed script of small calls through every list and frame launcher, for comparing the kernel dispatches of two builds of the library.

Run it twice under the kernel trace, alone (no counters, no other tracing), and compare the two traces:

  CGRT_LIB_NAME=libcgrt_parent.so rocprofv3 --kernel-trace --output-format csv -d DIR_A -o t -- python tools/trace_dispatches.py
  rocprofv3 --kernel-trace --output-format csv -d DIR_B -o t -- python tools/trace_dispatches.py
  python tools/trace_dispatches.py --compare DIR_A DIR_B --out profiles/NAME_dispatches.txt

The comparison is of the multiset of (kernel name, grid size, workgroup size, LDS bytes) -- a multiset because a frame's streams
interleave; its exit status is 1 when the two differ.  Frame hints are off (their grids depend on measured wave times) and
CGRT_STRIDED_WAVES is 64, so that the cap of the enqueued frames' grids binds at these sizes.  On the 20 K dragon stand-in and the
Cornell fixture, each with the certified and the exact walk: intersect of 4 096, 8 193, 65 536 and 200 000 rays under every kernel
shape (by size, then forced 0..3), occluded, in_shadow and shade_rays of 4 096 items, a 128 x 128 depth-3 frame twice (the exact path,
then the predicted one with its paired launch), spherical lights, two views, two light sets, two views x two light sets with a spherical
light, geometry buffers, and the enqueued form of each that has one."""
import argparse
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 128
DEPTH = 3
SAMPLES = 8


def run():
    os.environ["CGRT_STRIDED_WAVES"] = "64"  # (read once per process, by the first capped launch)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch  # (first: torch's HIP runtime is the one libcgrt.so binds to)

    import __graft_entry__ as entry

    pkg = entry.load_package()
    pkg.set_frame_hints(0)
    cam = pkg.scenes.default_camera(W, H).astype(np.float32)
    cams = np.stack([cam, cam])
    cams[1, 3] += np.float32(0.04)
    cams[1, 4] -= np.float32(0.09)
    sph = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    sph2 = sph.copy()
    sph2[0, 0:3] += np.float32([0.2, -0.05, 0.1])
    units = pkg.unit_vector_table(1 << 10)
    points = np.random.default_rng(7).uniform(-0.5, 0.5, (4096, 3)).astype(np.float32)
    scenes = {"dragon20k": pkg.scenes.make_dragon(20_000),
              "cornell": pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", "cornell.npz"))}
    for name, sd in scenes.items():
        L = np.ascontiguousarray(np.asarray(sd.point_lights, np.float32).reshape(-1, 6))
        moved = L.copy()
        moved[:, 0:3] += np.float32([0.25, 0.1, -0.2])
        sets = [L, np.concatenate([L, moved])]
        for certified in (True, False):
            sc = pkg.Scene(sd, device=0)  # (a fresh scene: its first frame takes the exact path, its second the predicted one)
            sc.set_walk(certified)
            rays = sc.generate_rays(pkg.scenes.default_camera(512, 512), 512, 512)
            for shape in (-1, 0, 1, 2, 3):
                pkg.set_kernel_shape(shape)
                for n in (4096, 8193, 65536, 200000):
                    sc.intersect(rays[:n])
            pkg.set_kernel_shape(-1)
            sc.occluded(rays[:4096])
            sc.in_shadow(points)
            sc.shade_rays(rays[:4096], max_level=DEPTH)
            for _ in range(2):
                sc.render(cam, W, H, max_level=DEPTH)
            sc.render_soft(cam, W, H, sph, units, samples=SAMPLES, max_level=DEPTH)
            sc.render_views(cams, W, H, max_level=DEPTH)
            sc.render_light_sets(cam, W, H, sets, max_level=DEPTH)
            sc.render_views_light_sets(cams, W, H, sets, spherical_sets=[sph, sph2], units=units, samples=SAMPLES, max_level=DEPTH)
            sc.render_aov_tensor(cam, W, H, max_level=DEPTH)
            torch.cuda.synchronize()
            # the enqueued forms
            d_rays = torch.from_numpy(np.ascontiguousarray(rays[:4096]).view(np.float32).reshape(-1, 7).copy()).cuda()
            sc.enqueue_render_tensor(cam, W, H, max_level=DEPTH)
            sc.enqueue_render_tensor(cam, W, H, max_level=DEPTH, spherical=sph, units=units, samples=SAMPLES)
            sc.enqueue_render_views_tensor(cams, W, H, max_level=DEPTH)
            sc.enqueue_render_views_light_sets_tensor(cams[:1], W, H, sets, max_level=DEPTH)
            sc.enqueue_render_views_light_sets_tensor(cams, W, H, sets, spherical_sets=[sph, sph2], units=units, samples=SAMPLES, max_level=DEPTH)
            sc.enqueue_shade_rays_tensor(d_rays, max_level=DEPTH)
            sc.enqueue_render_aov_tensor(cam, W, H, max_level=DEPTH)
            torch.cuda.synchronize()
            sc.close()
            print(f"{name} {'certified' if certified else 'exact'} walk: done", flush=True)


def dispatches(trace_dir):
    """Counter of (kernel name, grid, workgroup, LDS bytes) over every *kernel_trace.csv under trace_dir."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_trace.csv under {trace_dir}")
    rows = collections.Counter()
    for fn in files:
        with open(fn, newline="") as f:
            for r in csv.DictReader(f):
                dims = lambda p: "x".join(r[k] for k in (p + "_X", p + "_Y", p + "_Z") if k in r) or r.get(p, "?")  # noqa: E731
                lds = next((r[k] for k in r if k.startswith("LDS")), "?")
                rows[(r["Kernel_Name"], dims("Grid_Size"), dims("Workgroup_Size"), lds)] += 1
    return rows


def compare(dir_a, dir_b, out):
    a, b = dispatches(dir_a), dispatches(dir_b)
    diff = sorted(k for k in set(a) | set(b) if a[k] != b[k])
    lines = ["tools/trace_dispatches.py under rocprofv3 --kernel-trace, the parent's library (A) against this tree's (B): the multiset of",
             "(kernel name, grid size, workgroup size, LDS bytes) over every dispatch of the run.", "",
             f"dispatches: A {sum(a.values())}, B {sum(b.values())} (of the library's own kernels: "
             f"A {sum(v for k, v in a.items() if 'cgrt::' in k[0])}, B {sum(v for k, v in b.items() if 'cgrt::' in k[0])})",
             f"distinct rows: A {len(a)}, B {len(b)}", f"differences: {len(diff)}"]
    lines += [f"  A x{a[k]:<5} B x{b[k]:<5} grid {k[1]} workgroup {k[2]} LDS {k[3]}  {k[0]}" for k in diff]
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text, end="")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"), help="compare two trace directories instead of running the calls")
    ap.add_argument("--out", help="file the comparison is written to")
    a = ap.parse_args()
    sys.exit(compare(a.compare[0], a.compare[1], a.out) if a.compare else run())

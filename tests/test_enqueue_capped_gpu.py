"""GPU: enqueued frames with the count-driven grids at their smallest cap.

At the default cap (CGRT_STRIDED_WAVES = 6144 waves) every list of tests/test_enqueue_gpu.py fits one pass of its launch, so the stride
loops never take a second step there.  Here a child process runs with CGRT_STRIDED_WAVES=64 (the knob is read once per process): a trace
launch then covers 64 workgroups -- 4096 rays per pass in LANE64, 1024 in LANE16, 16 workgroups of 256 threads for the exact walk -- and a
shading launch 4096 threads, so every list above a few thousand entries strides.  The child checks enqueued against blocking bytes, whole
buffers with their sentinels, for 0, 1 and 2 lights, depth 2, 4 and 16, spherical lights, aa, rank 1 of 3 and all ranks merged, views, a ray
list written just before the call, the exact walk and a forced LANE16 shape, and a frame whose deeper lists take the device's LANE16 choice
past the cap."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 64
PAD = 4096


def test_enqueued_bytes_with_the_smallest_cap():
    pytest.importorskip("torch")
    env = dict(os.environ, CGRT_STRIDED_WAVES=str(CAP))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "capped cases ok" in r.stdout, r.stdout[-2000:]


# ---- the child process ----
def _child():
    sys.path.insert(0, ROOT)
    import torch  # (first: torch's HIP runtime is the one libcgrt.so binds to)

    import __graft_entry__ as entry

    pkg = entry.load_package()
    assert pkg.lib().cgrt_debug_strided_waves() == CAP, "the cap was not taken from CGRT_STRIDED_WAVES"

    def load(name):
        return pkg.scenes.SceneData.load(os.path.join(ROOT, "tests", "golden", "scenes", name + ".npz"))

    def fenced(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[PAD:PAD + nbytes].view(dtype).view(shape)

    def lights(sd, k):
        if k == 0:
            return np.zeros((0, 6), np.float32)
        base = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)[:1]
        if len(base) == 0:
            base = np.asarray([[0.0, 2.0, 2.0, 1.0, 1.0, 1.0]], np.float32)
        extra = base.copy()
        extra[0, :3] += np.float32([0.7, 0.3, -0.4])
        return np.ascontiguousarray(np.concatenate([base, extra])[:k])

    def moved(W, H, i):
        cam = pkg.scenes.default_camera(W, H).copy()
        cam[3] += np.float32(0.03 * i)
        cam[4] += np.float32(0.05 * i)
        return cam

    def same_frame(sc, cam, W, H, what, **kw):
        b_e, o_e = fenced((H, W, 3), torch.float32)
        b_b, o_b = fenced((H, W, 3), torch.float32)
        _, t = sc.enqueue_render_tensor(cam, W, H, out=o_e, **kw)
        _, st = sc.render_tensor(cam, W, H, out=o_b, **kw)
        torch.cuda.synchronize()
        assert torch.equal(b_e, b_b), what
        est = sc.enqueue_stats(t)
        for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels", "soft_shadow_rays"):
            assert est[k] == st[k], (what, k, est, st)
        return est

    cornell, monkey = pkg.Scene(load("cornell"), device=0), pkg.Scene(load("monkey"), device=0)
    W, H = 160, 120  # 19 200 primary rays: level 0's lists take 5 passes in LANE64, deeper ones several in LANE16
    for sc, name in ((cornell, "cornell"), (monkey, "monkey")):
        cam = pkg.scenes.default_camera(W, H)
        for depth in (2, 4, 16):
            for nl in (0, 1, 2):  # (0 lights: the mirror lists go out alone, k_trace_batch; with lights, paired with the shadow lists)
                same_frame(sc, cam, W, H, f"{name} depth {depth} lights {nl}", lights=lights(sc.sd, nl), max_level=depth)
    # lists of at most 131 072 entries take LANE16 on the device (16 rays per workgroup: 1024 per pass here).  Cornell's level-1 list held
    # 1 286 mirror rays at 320x240, so at 480x360 it holds more than 1 024 (checked): the deeper list itself strides past the cap in LANE16.
    est = same_frame(cornell, pkg.scenes.default_camera(480, 360), 480, 360, "cornell 480x360 depth 4", max_level=4, lights=lights(cornell.sd, 1))
    print("cornell 480x360 depth 4:", est)
    assert est["reflection_rays"] > 1024 and est["levels"] >= 2, est
    cam = pkg.scenes.default_camera(W, H)
    units = pkg.unit_vector_table(4096, 3)
    two = np.concatenate([pkg.scenes.CORNELL_SPHERICAL_LIGHTS, pkg.scenes.CORNELL_SPHERICAL_LIGHTS + np.float32([0.2, 0, 0.1, 0, 0, 0, 0])])
    same_frame(cornell, cam, W, H, "spherical lights", max_level=3, spherical=two, units=units, samples=8, seed=5)
    same_frame(cornell, cam, W, H, "aa", max_level=4, aa=True)
    same_frame(cornell, cam, W, H, "rank 1 of 3", max_level=4, rank=1, nranks=3)
    b_m, o_m = fenced((H, W, 3), torch.float32)
    for r in range(3):
        cornell.enqueue_render_tensor(cam, W, H, out=o_m, max_level=4, rank=r, nranks=3, aa=True)
    b_b, o_b = fenced((H, W, 3), torch.float32)
    cornell.render_tensor(cam, W, H, out=o_b, max_level=4, aa=True)
    torch.cuda.synchronize()
    assert torch.equal(b_m, b_b), "three aa ranks merged"
    # views
    VW, VH, B = 96, 64, 5
    cams = np.stack([moved(VW, VH, i) for i in range(B)])
    for kw in (dict(max_level=4, lights=lights(cornell.sd, 2)), dict(max_level=2, spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS, units=units,
                                                                      samples=4, seed=3)):
        b_e, o_e = fenced((B, VH, VW, 3), torch.float32)
        b_b, o_b = fenced((B, VH, VW, 3), torch.float32)
        cornell.enqueue_render_views_tensor(cams, VW, VH, out=o_e, **kw)
        cornell.render_views_tensor(cams, VW, VH, out=o_b, **kw)
        torch.cuda.synchronize()
        assert torch.equal(b_e, b_b), ("views", sorted(kw))
    # a ray list written by a torch op on the stream right before the call
    src = torch.from_numpy(np.ascontiguousarray(monkey.generate_rays(cam, W, H)).view(np.float32).reshape(H, W, 7).copy()).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rays = torch.empty_like(src)
        b_e, o_e = fenced((H, W, 3), torch.float32)
        b_b, o_b = fenced((H, W, 3), torch.float32)
        rays.copy_(src * 1.0)
        monkey.enqueue_shade_rays_tensor(rays, out=o_e, stream=s, lights=lights(monkey.sd, 2), max_level=4)
        monkey.shade_rays_tensor(rays, out=o_b, stream=s, lights=lights(monkey.sd, 2), max_level=4)
    s.synchronize()
    assert torch.equal(b_e, b_b), "ray list"
    # a forced LANE16 shape, then the exact walk (256-thread workgroups)
    try:
        pkg.set_kernel_shape(2)
        same_frame(monkey, cam, W, H, "forced LANE16", max_level=4, lights=lights(monkey.sd, 2))
    finally:
        pkg.set_kernel_shape(-1)
    for sc, name in ((monkey, "monkey"), (cornell, "cornell")):
        sc.set_walk(False)
        try:
            same_frame(sc, cam, W, H, f"{name} exact walk", max_level=4, lights=lights(sc.sd, 2))
        finally:
            sc.set_walk(True)
    cornell.close()
    monkey.close()
    print("capped cases ok")


if __name__ == "__main__":
    _child()

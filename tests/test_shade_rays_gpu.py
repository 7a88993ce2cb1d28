"""GPU tests of getFinalColor for caller-supplied rays (cgrt_shade_rays / cgrt_shade_rays_device / Scene.shade_rays*).

* The camera's own rays, as a list, give the camera's frame bit for bit (plain, soft shadows, anti-aliased sub-samples), with the
  same ray counts.
* A ray's colour depends on nothing but the ray: not on the list's length, order or kernel shape, nor on the walk.
* Arbitrary rays (inside and outside the Cornell box, non-unit directions, finite t) agree with the C++ mirror's literal per-ray
  recursion within the RGB parity bar, with equal ray counts.
* The device entry: bit-identical to the host entry, any leading shape, writes exactly its output, orders on the caller's stream,
  refuses memory that is not the scene's device memory before any work.
* Camera frames around a ray list behave as without it (prediction, render_tensor's output)."""
import ctypes as C
import time

import numpy as np
import pytest
import rayfam

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -1
PREDICTED = 1
SHAPES = (-1, 0, 1, 2, 3)  # cgrt_set_kernel_shape: auto, LANE64, QUAD16, LANE16, QUAD4


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _cam(pkg, name, W, H):
    if name == "spheres":  # (as tests/test_antialias_gpu.py)
        return np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
    return pkg.scenes.default_camera(W, H)


def _soft(pkg, samples=16, seed=11):
    return dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(4096, 3), samples=samples, seed=seed)


_COUNTS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays")


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    made = {n: pkg.Scene(scene_data(n), device=0) for n in ("cube", "monkey", "spheres", "cornell")}
    yield made
    for s in made.values():
        s.close()


@pytest.mark.parametrize("name", ["cube", "monkey", "spheres", "cornell"])
@pytest.mark.parametrize("W,H", [(97, 61), (1, 1), (3, 1), (800, 800)])
def test_camera_rays_equal_the_frame(pkg, scenes, name, W, H):
    sc = scenes[name]
    cam = _cam(pkg, name, W, H)
    rays = sc.generate_rays(cam, W, H)
    soft = _soft(pkg)
    for depth in (0, 1, 2, 4):
        want, wst = sc.render(cam, W, H, max_level=depth)
        got, gst = sc.shade_rays(rays, max_level=depth)
        assert _same_bits(got, want), (name, W, H, depth)
        assert all(gst[k] == wst[k] for k in _COUNTS), (gst, wst)
        assert gst["primary_rays"] == (W * H if depth >= 1 else 0)
        want, wst = sc.render_soft(cam, W, H, max_level=depth, **soft)
        got, gst = sc.shade_rays(rays, max_level=depth, **soft)
        assert _same_bits(got, want), ("soft", name, W, H, depth)
        assert all(gst[k] == wst[k] for k in _COUNTS), (gst, wst)


@pytest.mark.parametrize("name", ["monkey", "cornell"])
def test_sub_sample_rays_resolved_equal_render_aa(pkg, scenes, name):
    sc = scenes[name]
    W, H = 97, 61
    cam = _cam(pkg, name, W, H)
    rays = sc.generate_rays(cam, 2 * W, 2 * H)  # (render_aa shades the 2W x 2H frame of the same camera)
    for depth, soft in ((2, None), (4, None), (2, _soft(pkg))):
        kw = soft or {}
        want, _ = sc.render_aa(cam, W, H, max_level=depth, **kw)
        sub, _ = sc.shade_rays(rays, max_level=depth, **kw)
        assert _same_bits(pkg.resolve_aa(sub, W, H), want), (name, depth, soft is not None)


def test_colour_depends_on_the_ray_only(pkg, scenes):
    """Random subsets and permutations of a Cornell frame's rays, under every forced kernel shape and both walks: each ray's colour is
    its pixel's colour in the full frame (a permutation only permutes the output)."""
    sc = scenes["cornell"]
    W, H = 640, 480  # 307 200 rays
    cam = pkg.scenes.default_camera(W, H)
    rays = sc.generate_rays(cam, W, H)
    rng = np.random.default_rng(5)
    lists = [rng.choice(W * H, k, replace=False) for k in (1, 63, 4096, 8193, 131073)] + [rng.permutation(W * H)]
    try:
        for certified in (True, False):
            sc.set_walk(certified)
            for depth in (2, 4):
                frame, _ = sc.render(cam, W, H, max_level=depth)
                for mode in SHAPES:
                    pkg.set_kernel_shape(mode)
                    for idx in lists:
                        got, st = sc.shade_rays(rays[idx], max_level=depth)
                        assert _same_bits(got, frame[idx]), (certified, depth, mode, len(idx))
                        assert st["primary_rays"] == len(idx)
                    pkg.set_kernel_shape(-1)
    finally:
        pkg.set_kernel_shape(-1)
        sc.set_walk(True)


@pytest.mark.parametrize("spherical", [False, True])
def test_arbitrary_rays_match_the_per_ray_recursion(pkg, scene_data, spherical):
    sd = scene_data("cornell")
    rays, short = rayfam.arbitrary_rays(sd, 2400, 41 + spherical)
    soft = _soft(pkg, samples=8, seed=3) if spherical else {}
    sc = pkg.Scene(sd, device=0)
    for depth in (1, 2, 4):
        dev, dst = pkg.host_shade_rays(sd, rays, max_level=depth, driver="device", **soft)
        ref, rst = pkg.host_shade_rays(sd, rays, max_level=depth, driver="per_ray", **soft)
        err = float(np.abs(dev - ref).max())
        assert err <= 1e-5, (depth, spherical, err)
        for k in ("primary", "shadow", "reflection", "soft_shadow"):
            assert dst[k] == rst[k], (k, depth, dst, rst)
        assert ref[short].max() == 0.0 and dev[short].max() == 0.0, "t shorter than the first hit: black"
        assert (ref.max(1) > 0).sum() > len(rays) // 4, "most rays must reach something"
        lib_rgb, lst = sc.shade_rays(rays, max_level=depth, **soft)  # the library entry itself, on the Python side's scene
        assert float(np.abs(lib_rgb - ref).max()) <= 1e-5
        assert lst["shadow_rays"] == rst["shadow"] and lst["reflection_rays"] == rst["reflection"]
        if depth >= 2:
            assert rst["reflection"] > 0
    sc.close()


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_shade_rays_tensor(pkg, scenes):
    sc = scenes["cornell"]
    W, H = 160, 96
    cam = pkg.scenes.default_camera(W, H)
    rays = sc.generate_rays(cam, W, H).view(np.float32).reshape(-1, 7)
    want, wst = sc.shade_rays(rays, max_level=4)
    d_rays = torch.from_numpy(rays).to("cuda:0")
    flat, st = sc.shade_rays_tensor(d_rays, max_level=4)
    assert tuple(flat.shape) == (W * H, 3) and flat.dtype == torch.float32
    assert _same_bits(_host(flat), want) and all(st[k] == wst[k] for k in _COUNTS)
    img, _ = sc.shade_rays_tensor(d_rays.view(H, W, 7), max_level=4)
    assert tuple(img.shape) == (H, W, 3)
    assert _same_bits(_host(img).reshape(-1, 3), want)
    # out inside a sentinel-filled buffer: every element written, nothing around it
    buf = torch.full((W * H * 3 + 64,), -7.25, dtype=torch.float32, device="cuda:0")
    out = buf[32 : 32 + W * H * 3].view(H, W, 3)
    got, _ = sc.shade_rays_tensor(d_rays.view(H, W, 7), out=out, max_level=4)
    assert got.data_ptr() == out.data_ptr()
    b = _host(buf)
    assert (b[:32] == np.float32(-7.25)).all() and (b[-32:] == np.float32(-7.25)).all()
    assert _same_bits(b[32:-32].reshape(-1, 3), want)
    # n == 0: nothing is touched, stats are zero; max_level == 0: black, nothing traced
    empty = torch.full((0, 3), 5.0, device="cuda:0")
    _, st0 = sc.shade_rays_tensor(torch.zeros((0, 7), device="cuda:0"), out=empty)
    assert all(v == 0 for v in st0.values())
    rgb0, st0 = sc.shade_rays(np.zeros((0, 7), np.float32))
    assert rgb0.shape == (0, 3) and all(v == 0 for v in st0.values())
    out = torch.full((H, W, 3), 5.0, device="cuda:0")
    _, st0 = sc.shade_rays_tensor(d_rays.view(H, W, 7), out=out, max_level=0)
    assert not _host(out).any() and st0["primary_rays"] == 0 and st0["shadow_rays"] == 0 and st0["levels"] == 0
    rgb0, _ = sc.shade_rays(rays, max_level=0)
    assert not rgb0.any()


def _delay_cycles(ms):
    """torch.cuda._sleep cycles that keep a stream busy for about `ms` milliseconds, from a timed delay of 1 M cycles (as
    tests/test_render_device_gpu.py sizes its stream-hazard delay)."""
    s = torch.cuda.Stream(device=0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        torch.cuda._sleep(1_000_000)
        e1.record()
    e1.synchronize()
    per_ms = 1_000_000 / max(e0.elapsed_time(e1), 1e-3)
    return int(per_ms * ms)


def test_stream_order(pkg, scenes):
    """Rays written by a torch kernel on a non-blocking side stream held back by a bounded delay, shaded at once on that stream with no
    synchronisation: the call's kernels wait for the rays, and what the stream runs after the call sees the colours."""
    sc = scenes["cornell"]
    W, H = 200, 120
    cam = pkg.scenes.default_camera(W, H)
    rays = torch.from_numpy(sc.generate_rays(cam, W, H).view(np.float32).reshape(H, W, 7)).to("cuda:0")
    want, _ = sc.shade_rays_tensor(rays, max_level=2)
    want = _host(want)
    s = torch.cuda.Stream(device=0)
    warm = torch.empty((H, W, 3), device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc.shade_rays_tensor(rays, out=warm, stream=s, max_level=2)
    call_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    cycles = _delay_cycles(min(2000.0, max(100.0, 20.0 * call_ms)))
    d_rays = torch.zeros_like(rays)
    out = torch.full((H, W, 3), 3.0, device="cuda:0")
    after = torch.empty_like(out)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        d_rays.copy_(rays * 1.0)  # the rays are made by a kernel on the side stream, behind the delay
    pending = torch.cuda.Event()
    pending.record(s)
    assert not pending.query(), "the delay must still hold the rays back when the call is made"
    sc.shade_rays_tensor(d_rays, out=out, stream=s, max_level=2)
    with torch.cuda.stream(s):
        after.copy_(out)  # enqueued after the call: sees the colours
    assert _same_bits(_host(out), want)
    assert _same_bits(_host(after), want)


def test_device_entry_refuses_foreign_memory(pkg, scenes):
    sc = scenes["cube"]
    n = 64
    rays = np.zeros((n, 7), np.float32)
    rgb = np.full((n, 3), 5.0, np.float32)
    d_rays = torch.zeros((n, 7), device="cuda:0")
    d_rgb = torch.full((n, 3), 5.0, device="cuda:0")
    L = np.ascontiguousarray(sc.sd.point_lights, np.float32).reshape(-1, 6)

    def call(r, c, nn=n):
        st = pkg.RenderStats()
        return pkg.lib().cgrt_shade_rays_device(sc._h, C.c_void_p(r), nn, L.ctypes.data_as(C.c_void_p), len(L), None, 2, C.c_void_p(c), None,
                                                C.byref(st))

    assert call(rays.ctypes.data, d_rgb.data_ptr()) == E_ARG, "host rays"
    assert call(d_rays.data_ptr(), rgb.ctypes.data) == E_ARG, "host colours"
    assert call(d_rays.data_ptr() + 2, d_rgb.data_ptr()) == E_ARG, "unaligned rays"
    assert (rgb == 5.0).all() and (_host(d_rgb) == 5.0).all(), "nothing is written before the checks"
    if torch.cuda.device_count() > 1:
        other = torch.zeros((n, 3), device="cuda:1")
        assert call(d_rays.data_ptr(), other.data_ptr()) == E_ARG, "memory of another device"
        assert (_host(other) == 0).all()
    st = pkg.RenderStats(primary_rays=9, levels=9)
    assert pkg.lib().cgrt_shade_rays_device(sc._h, C.c_void_p(d_rays.data_ptr()), 0, None, 0, None, 2, C.c_void_p(d_rgb.data_ptr()), None,
                                            C.byref(st)) == 0, "n == 0 succeeds"
    assert st.primary_rays == 0 and st.levels == 0 and (_host(d_rgb) == 5.0).all(), "n == 0: zeroed stats, nothing touched"
    assert call(d_rays.data_ptr(), d_rgb.data_ptr()) == 0
    assert not _host(d_rgb).any(), "zero rays (direction 0) reach nothing: black"


def test_camera_frames_around_a_ray_list(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"), device=0)
    W, H = 160, 96
    cam = pkg.scenes.default_camera(W, H)
    other = pkg.scenes.default_camera(W, H).copy()
    other[4] += np.float32(0.2)
    a, _ = sc.render(cam, W, H)
    b, _ = sc.render(cam, W, H)
    assert sc.last_render_path() == PREDICTED and _same_bits(a, b)
    sc.shade_rays(sc.generate_rays(other, 97, 61), max_level=4)  # another size and depth: a frame would reset the prediction
    c, _ = sc.render(cam, W, H)
    assert sc.last_render_path() == PREDICTED, "the ray list neither reads nor writes the frame prediction"
    assert _same_bits(c, b)
    # a ray list right after render_tensor leaves that tensor's contents correct
    t, _ = sc.render_tensor(cam, W, H)
    sc.shade_rays(sc.generate_rays(other, W, H), max_level=4)
    assert _same_bits(_host(t).reshape(-1, 3), a)
    sc.close()

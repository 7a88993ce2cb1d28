"""GPU tests of enqueued frames (include/cgrt.h cgrt_enqueue_*, Scene.enqueue_*).

* Bytes: every enqueued frame, view batch and ray list writes exactly the bytes of its blocking counterpart (render_tensor,
  render_views_tensor, shade_rays_tensor) for the same arguments, into buffers that sit between sentinel bytes: the whole buffers, sentinels
  included, are compared.
* Stream order without waiting: the call returns while the stream is still busy with a long sleep, and the frame still runs behind the
  torch op the caller queued before it.
* Frames in flight: 3 x 8 enqueued frames on two streams, blocking frames in between, one synchronise; a predicted blocking frame stays
  predicted and byte-identical around them; closing the scene with frames in flight completes them.
* Tickets: enqueue_stats equals the blocking call's ray counts and levels; an expired or unknown ticket is CGRT_E_ARG."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

E_ARG = -1
PAD = 4096  # sentinel bytes on each side of an output
SENTINEL = 0xA5


def _cam(pkg, name, W, H):
    if name == "spheres":  # (as tests/test_render_device_gpu.py)
        return np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
    return pkg.scenes.default_camera(W, H)


def _moved(pkg, W, H, i):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[3] += np.float32(0.03 * i)
    cam[4] += np.float32(0.05 * i)
    return cam


def _lights(sd, k):
    base = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    if k == 0:
        return np.zeros((0, 6), np.float32)
    if len(base) == 0:
        base = np.asarray([[0.0, 2.0, 2.0, 1.0, 1.0, 1.0]], np.float32)
    extra = base[:1].copy()
    extra[0, :3] += np.float32([0.7, 0.3, -0.4])
    extra[0, 3:] = np.float32([0.5, 0.8, 0.6])
    return np.ascontiguousarray(np.concatenate([base, extra])[:k])


def _fenced(shape, dtype):
    """(whole buffer filled with sentinel bytes, the output view in its middle)"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((PAD + nbytes + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf[PAD:PAD + nbytes].view(dtype).view(shape)


def _pitched(W, H, extra=7):
    """an (H, W, 3) f32 view with a row pitch of (W + extra) pixels, between sentinels"""
    buf = torch.full((PAD + H * (W + extra) * 12 + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rows = buf[PAD:PAD + H * (W + extra) * 12].view(torch.float32).view(H, W + extra, 3)
    return buf, rows[:, :W, :]


_FMT = {"rgb": (lambda W, H: (H, W, 3), torch.float32), "chw": (lambda W, H: (3, H, W), torch.float32), "rgba8": (lambda W, H: (H, W, 4), torch.uint8)}


def _same_frame(sc, cam, W, H, fmt="rgb", **kw):
    """enqueue_render_tensor and render_tensor into fenced buffers: the buffers are byte-identical"""
    shape, dtype = _FMT[fmt]
    b_enq, o_enq = _fenced(shape(W, H), dtype)
    b_blk, o_blk = _fenced(shape(W, H), dtype)
    _, ticket = sc.enqueue_render_tensor(cam, W, H, format=fmt, out=o_enq, **kw)
    _, st = sc.render_tensor(cam, W, H, format=fmt, out=o_blk, **kw)
    torch.cuda.synchronize()
    assert torch.equal(b_enq, b_blk), (fmt, kw.get("max_level"), kw.get("aa"))
    est = sc.enqueue_stats(ticket)
    for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels", "soft_shadow_rays"):
        assert est[k] == st[k], (k, est, st)


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    out = {name: pkg.Scene(scene_data(name), device=0) for name in ("cube", "monkey", "spheres", "cornell")}
    out["dragon"] = pkg.Scene(pkg.scenes.make_dragon(50_000), device=0)
    yield out
    for s in out.values():
        s.close()


@pytest.mark.parametrize("name", ["cube", "monkey", "spheres", "cornell", "dragon"])
def test_frames_equal_the_blocking_entry(pkg, scenes, name):
    sc = scenes[name]
    W, H = 96, 64
    cam = _cam(pkg, name, W, H)
    for depth in (0, 1, 2, 4, 16):
        for nl in (0, 1, 2):
            _same_frame(sc, cam, W, H, lights=_lights(sc.sd, nl), max_level=depth)


def test_frame_variants_equal_the_blocking_entry(pkg, scenes):
    sc = scenes["cornell"]
    W, H = 80, 72
    cam = _cam(pkg, "cornell", W, H)
    units = pkg.unit_vector_table(4096, 3)
    two = np.concatenate([pkg.scenes.CORNELL_SPHERICAL_LIGHTS, pkg.scenes.CORNELL_SPHERICAL_LIGHTS + np.float32([0.2, 0, 0.1, 0, 0, 0, 0])])
    for samples in (1, 200):
        for sph in (pkg.scenes.CORNELL_SPHERICAL_LIGHTS, two):
            _same_frame(sc, cam, W, H, max_level=2, spherical=sph, units=units, samples=samples, seed=5)
    _same_frame(sc, cam, W, H, max_level=4, spherical=two, units=units, samples=16, seed=1, aa=True)
    for fmt in ("rgb", "chw", "rgba8"):
        for aa in (False, True):
            _same_frame(sc, cam, W, H, fmt=fmt, max_level=3, aa=aa)
    # a row pitch
    b_enq, o_enq = _pitched(W, H)
    b_blk, o_blk = _pitched(W, H)
    sc.enqueue_render_tensor(cam, W, H, out=o_enq, max_level=2)
    sc.render_tensor(cam, W, H, out=o_blk, max_level=2)
    torch.cuda.synchronize()
    assert torch.equal(b_enq, b_blk)
    # rank 1 of 3 alone, and all three ranks merged into one buffer, with and without aa
    for aa in (False, True):
        _same_frame(sc, cam, W, H, max_level=2, rank=1, nranks=3, aa=aa)
        b_m, o_m = _fenced((H, W, 3), torch.float32)
        for r in range(3):
            sc.enqueue_render_tensor(cam, W, H, out=o_m, max_level=2, rank=r, nranks=3, aa=aa)
        b_blk, o_blk = _fenced((H, W, 3), torch.float32)
        sc.render_tensor(cam, W, H, out=o_blk, max_level=2, aa=aa)
        torch.cuda.synchronize()
        assert torch.equal(b_m, b_blk), aa
    # a camera that sees nothing, right after one that sees the scene
    away = cam.copy()
    away[3] += np.float32(np.pi)
    _same_frame(sc, cam, W, H, max_level=3)
    _same_frame(sc, away, W, H, max_level=3)


def test_exact_walk_and_forced_shapes(pkg, scenes):
    sc = scenes["monkey"]
    W, H = 64, 64
    cam = _cam(pkg, "monkey", W, H)
    try:
        for mode in (2, 0, 3):  # LANE16, LANE64, QUAD4 for every list
            pkg.set_kernel_shape(mode)
            _same_frame(sc, cam, W, H, max_level=4, lights=_lights(sc.sd, 2))
    finally:
        pkg.set_kernel_shape(-1)
    sc.set_walk(False)
    try:
        _same_frame(sc, cam, W, H, max_level=4, lights=_lights(sc.sd, 2))
    finally:
        sc.set_walk(True)


@pytest.mark.parametrize("B", [1, 5, 16])
def test_views_equal_the_blocking_entry(pkg, scenes, B):
    sc = scenes["cornell"]
    W, H = 48, 40
    cams = np.stack([_moved(pkg, W, H, i) for i in range(B)])
    units = pkg.unit_vector_table(1024, 2)
    for kw in (dict(max_level=0), dict(max_level=2), dict(max_level=4, lights=_lights(sc.sd, 2)),
               dict(max_level=2, spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS, units=units, samples=8, seed=3)):
        for fmt in ("rgb", "rgba8"):
            shape, dtype = _FMT[fmt]
            b_enq, o_enq = _fenced((B,) + shape(W, H), dtype)
            b_blk, o_blk = _fenced((B,) + shape(W, H), dtype)
            _, t = sc.enqueue_render_views_tensor(cams, W, H, format=fmt, out=o_enq, **kw)
            _, st = sc.render_views_tensor(cams, W, H, format=fmt, out=o_blk, **kw)
            torch.cuda.synchronize()
            assert torch.equal(b_enq, b_blk), (fmt, kw.keys())
            est = sc.enqueue_stats(t)
            assert (est["shadow_rays"], est["reflection_rays"], est["levels"]) == (st["shadow_rays"], st["reflection_rays"], st["levels"])


def _rays_of(sc, cam, W, H):
    return torch.from_numpy(np.ascontiguousarray(sc.generate_rays(cam, W, H)).view(np.float32).reshape(H, W, 7).copy())


def test_ray_lists_equal_the_blocking_entry(pkg, scenes):
    for name in ("cornell", "monkey", "dragon"):
        sc = scenes[name]
        W, H = 72, 56
        src = _rays_of(sc, _cam(pkg, name, W, H), W, H).cuda()
        for depth in (0, 1, 2, 4):
            for nl in (0, 2):
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    rays = torch.empty_like(src)
                    b_enq, o_enq = _fenced((H, W, 3), torch.float32)
                    b_blk, o_blk = _fenced((H, W, 3), torch.float32)
                    rays.copy_(src * 1.0)  # (written by a torch op on the stream, right before the call)
                    _, t = sc.enqueue_shade_rays_tensor(rays, out=o_enq, stream=s, lights=_lights(sc.sd, nl), max_level=depth)
                    _, st = sc.shade_rays_tensor(rays, out=o_blk, stream=s, lights=_lights(sc.sd, nl), max_level=depth)
                s.synchronize()
                assert torch.equal(b_enq, b_blk), (name, depth, nl)
                est = sc.enqueue_stats(t)
                for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels"):
                    assert est[k] == st[k], (k, est, st)


def _sleep_cycles(seconds):
    return int(seconds * 1e9 * 2.4)  # (~2.4 GHz shader clock; only the order of magnitude matters)


@pytest.mark.parametrize("kind", ["frame", "views", "rays"])
def test_call_does_not_wait_and_frame_waits_for_the_stream(pkg, scenes, kind):
    sc = scenes["cornell"]
    W, H = 128, 96
    cam = _cam(pkg, "cornell", W, H)
    cams = np.stack([_moved(pkg, W, H, i) for i in range(3)])
    src = _rays_of(sc, cam, W, H).cuda()
    s = torch.cuda.Stream()
    shape = (3, H, W, 3) if kind == "views" else (H, W, 3)
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    ref = torch.empty(shape, dtype=torch.float32, device="cuda")
    rays = torch.empty_like(src)

    def call():
        if kind == "frame":
            return sc.enqueue_render_tensor(cam, W, H, out=out, stream=s, max_level=3)
        if kind == "views":
            return sc.enqueue_render_views_tensor(cams, W, H, out=out, stream=s, max_level=3)
        return sc.enqueue_shade_rays_tensor(rays, out=out, stream=s, max_level=3)

    with torch.cuda.stream(s):
        rays.copy_(src)
        if kind == "frame":
            sc.render_tensor(cam, W, H, out=ref, stream=s, max_level=3)
        elif kind == "views":
            sc.render_views_tensor(cams, W, H, out=ref, stream=s, max_level=3)
        else:
            sc.shade_rays_tensor(rays, out=ref, stream=s, max_level=3)
        call()  # (warm: the workspace has its size)
    s.synchronize()
    with torch.cuda.stream(s):
        rays.zero_()
        torch.cuda._sleep(_sleep_cycles(0.2))
        if kind == "rays":
            rays.copy_(src)  # (the rays are written behind the sleep)
        else:
            out.fill_(float("nan"))  # (the frame must overwrite this, so it ran behind it)
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        ev = torch.cuda.Event()
        ev.record(s)
    pending = not ev.query()
    s.synchronize()
    assert dt < 0.05, f"the enqueue call took {dt * 1e3:.1f} ms"
    assert pending, "the stream had finished when the call returned"
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "the frame did not run behind the fill"


def test_many_frames_in_flight(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"), device=0)
    W, H = 96, 80
    cam0 = pkg.scenes.default_camera(W, H)
    # a predicted blocking frame before the run
    sc.render_tensor(cam0, W, H, max_level=2)
    pre, _ = sc.render_tensor(cam0, W, H, max_level=2)
    torch.cuda.synchronize()
    assert sc.last_render_path() == 1
    pre = pre.clone()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs, blocking = [], []
    for i in range(24):
        s = streams[i % 2]
        with torch.cuda.stream(s):
            o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            o.record_stream(s)
        sc.enqueue_render_tensor(_moved(pkg, W, H, i), W, H, out=o, stream=s, max_level=3)
        outs.append(o)
        if i % 5 == 4:
            b, _ = sc.render_tensor(_moved(pkg, W, H, 100 + i), W, H, stream=s, max_level=3)
            blocking.append((100 + i, b))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        ref, _ = sc.render_tensor(_moved(pkg, W, H, i), W, H, max_level=3)
        torch.cuda.synchronize()
        assert torch.equal(o, ref), i
    for i, b in blocking:
        ref, _ = sc.render_tensor(_moved(pkg, W, H, i), W, H, max_level=3)
        torch.cuda.synchronize()
        assert torch.equal(b, ref), i
    # the predicted frame after the run: same path, same bytes
    sc.render_tensor(cam0, W, H, max_level=2)
    post, _ = sc.render_tensor(cam0, W, H, max_level=2)
    torch.cuda.synchronize()
    assert sc.last_render_path() == 1
    assert torch.equal(post, pre)
    # closing the scene with frames in flight completes them
    late = []
    for i in range(6):
        o, _ = sc.enqueue_render_tensor(_moved(pkg, W, H, i), W, H, stream=streams[0], max_level=3)
        late.append(o)
    sc.close()
    streams[0].synchronize()
    for i, o in enumerate(late):
        assert torch.equal(o, outs[i]), i


def test_tickets(pkg, scenes):
    sc = scenes["cube"]
    W, H = 64, 48
    cam = _cam(pkg, "cube", W, H)
    tickets = []
    for i in range(10):
        _, t = sc.enqueue_render_tensor(cam, W, H, max_level=2)
        tickets.append(t)
    assert tickets == sorted(tickets) and len(set(tickets)) == 10
    _, st = sc.render_tensor(cam, W, H, max_level=2)
    est = sc.enqueue_stats(tickets[-1])
    for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels"):
        assert est[k] == st[k]
    assert est["device_ms"] > 0
    for bad in (tickets[0], tickets[1], 0, tickets[-1] + 1000):  # (out of the ring of 8, never issued)
        with pytest.raises(pkg.CgrtError) as e:
            sc.enqueue_stats(bad)
        assert e.value.code == E_ARG

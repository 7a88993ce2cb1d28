"""GPU tests of multi-view frames (include/cgrt.h cgrt_trace_primary_views_device, cgrt_render_views, cgrt_render_views_device;
Scene.trace_views_device / render_views / render_views_tensor).

View b of a batch must be, bit for bit, the single-camera frame of cams[b]: hits and normals of trace_primary_device, RGB of render /
render_soft / render_tensor in every format.  Every device output is surrounded by sentinel bytes that must survive.  A batch must
leave the scene's single-camera state alone (prediction record, frame hints), order itself behind the caller's stream, and agree
with the CPU oracle."""
import numpy as np
import pytest

from conftest import same_bits as _same_bits_elementwise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORMATS = ("rgb", "chw", "rgba8")


def same_bits(a, b):
    """Every element bit-identical (NaN payloads aside: conftest.same_bits)."""
    return np.shape(a) == np.shape(b) and bool(_same_bits_elementwise(a, b).all())
EXACT, PREDICTED = 0, 1
SENTINEL = 0xA5


def _cams(pkg, B, W, H, spread=1.0):
    """B cameras around the default one that differ in euler, distance, fovy and aspect."""
    base = pkg.scenes.default_camera(max(W, 1), max(H, 1)).astype(np.float32)
    a = np.repeat(base[None, :], B, axis=0)
    k = np.arange(B, dtype=np.float32)
    a[:, 3] += np.float32(0.04 * spread) * k
    a[:, 4] += np.float32(-0.09 * spread) * k
    a[:, 6] *= np.float32(1.0) + np.float32(0.07) * k
    a[:, 7] *= np.float32(1.0) - np.float32(0.03) * k
    a[:, 8] *= np.float32(1.0) + np.float32(0.05) * (k % 3)
    return np.ascontiguousarray(a, np.float32)


def _guarded(nbytes, dtype=torch.uint8, pad=256):
    """(buffer with sentinel bytes on both sides, the inner byte view, check())"""
    buf = torch.full((nbytes + 2 * pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    inner = buf[pad : pad + nbytes]

    def intact():
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        return bool((b[:pad] == SENTINEL).all() and (b[pad + nbytes :] == SENTINEL).all())

    return buf, inner, intact


def _hits_of(pkg, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(pkg.HIT_DTYPE)


def _trace_single(pkg, sc, cam, W, H):
    h = torch.full((W * H * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    n = torch.full((W * H * 12,), SENTINEL, dtype=torch.uint8, device="cuda")
    sc.trace_primary_device(cam, W, H, h.data_ptr(), d_normals_ptr=n.data_ptr())
    torch.cuda.synchronize()
    return h.cpu().numpy(), n.cpu().numpy()


def _trace_views(pkg, sc, cams, W, H):
    B = len(cams)
    hb, hi, hok = _guarded(B * W * H * 16)
    nb, ni, nok = _guarded(B * W * H * 12)
    sc.trace_views_device(cams, W, H, hi.data_ptr(), d_normals_ptr=ni.data_ptr())
    assert hok() and nok(), "bytes outside the batch's hits / normals were written"
    return hi.cpu().numpy().reshape(B, -1), ni.cpu().numpy().reshape(B, -1)


@pytest.fixture(scope="module")
def dragon(pkg):
    sc = pkg.Scene(pkg.scenes.make_dragon(20_000))
    assert sc.walk() == 1, "the stand-in has a fast tree (certified walk)"
    yield sc
    sc.close()


@pytest.mark.parametrize("certified", [True, False])
@pytest.mark.parametrize("shape", [-1, 1])  # auto (lane64 frames), quad16 (cgrt_set_kernel_shape)
def test_trace_views_equal_single_frames(pkg, dragon, certified, shape):
    sc = dragon
    sc.set_walk(certified)
    pkg.set_kernel_shape(shape)
    try:
        for W, H in ((1, 1), (5, 3), (67, 45), (200, 130)):
            for B in (1, 3, 7):
                cams = _cams(pkg, B, W, H)
                hv, nv = _trace_views(pkg, sc, cams, W, H)
                for b in range(B):
                    h1, n1 = _trace_single(pkg, sc, cams[b], W, H)
                    assert hv[b].tobytes() == h1.tobytes(), ("hits", W, H, B, b)
                    assert nv[b].tobytes() == n1.tobytes(), ("normals", W, H, B, b)
                hits = hv.view(pkg.HIT_DTYPE)
                if W * H > 100:
                    assert hits["hit"].any(), "the batch sees the scene"
        # a list of Camera works as the array does, and the normals are optional
        cams = _cams(pkg, 3, 67, 45)
        hb, hi, hok = _guarded(3 * 67 * 45 * 16)
        sc.trace_views_device([pkg.Camera.from_array(c) for c in cams], 67, 45, hi.data_ptr())
        assert hok()
        assert hi.cpu().numpy().tobytes() == _trace_views(pkg, sc, cams, 67, 45)[0].tobytes()
    finally:
        pkg.set_kernel_shape(-1)
        sc.set_walk(True)


def test_trace_views_cornell_exact_walk(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"))
    W, H = 67, 45
    cams = _cams(pkg, 7, W, H)
    hv, nv = _trace_views(pkg, sc, cams, W, H)
    for b in range(7):
        h1, n1 = _trace_single(pkg, sc, cams[b], W, H)
        assert hv[b].tobytes() == h1.tobytes() and nv[b].tobytes() == n1.tobytes(), b
    sc.close()


def _render_cam(pkg, name, W, H, B):
    if name == "spheres":  # (as tests/test_render_device_gpu.py)
        base = np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
        a = np.repeat(base[None, :], B, axis=0)
        a[:, 4] += np.float32(0.1) * np.arange(B, dtype=np.float32)
        a[:, 6] *= np.float32(1.0) + np.float32(0.05) * np.arange(B, dtype=np.float32)
        return np.ascontiguousarray(a)
    return _cams(pkg, B, W, H)


def _export_views(pkg, sc, cams, W, H, fmt, **kw):
    B = len(cams)
    per = W * H * (4 if fmt == "rgba8" else 12)
    buf, inner, intact = _guarded(B * per)
    shape = {"rgb": (B, H, W, 3), "chw": (B, 3, H, W), "rgba8": (B, H, W, 4)}[fmt]
    st = sc.render_views_device(cams, W, H, inner.data_ptr(), format=fmt, **kw)
    assert intact(), "bytes outside the batch's frames were written"
    a = inner.cpu().numpy()
    return (a if fmt == "rgba8" else a.view(np.float32)).reshape(shape), st


STAT_KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays")


@pytest.mark.parametrize("name", ["cube", "monkey", "spheres", "cornell"])
@pytest.mark.parametrize("depth", [0, 2, 4])
def test_render_views_equal_single_frames(pkg, scene_data, name, depth):
    sc = pkg.Scene(scene_data(name))
    W, H, B = 72, 40, 4
    cams = _render_cam(pkg, name, W, H, B)
    got, gst = sc.render_views(cams, W, H, max_level=depth)
    assert got.shape == (B, W * H, 3)
    singles = [sc.render(cams[b], W, H, max_level=depth) for b in range(B)]
    for b in range(B):
        assert same_bits(got[b], singles[b][0]), (name, depth, b)
    for k in STAT_KEYS:
        assert gst[k] == sum(s[1][k] for s in singles), k
    if depth >= 1:
        assert gst["primary_rays"] == B * W * H
    for fmt in FORMATS:
        out, st = _export_views(pkg, sc, cams, W, H, fmt, max_level=depth)
        t, tst = sc.render_views_tensor(cams, W, H, format=fmt, max_level=depth)
        torch.cuda.synchronize()
        assert tuple(t.shape) == out.shape and t.is_contiguous()
        assert t.cpu().numpy().tobytes() == out.tobytes(), fmt
        for k in STAT_KEYS:
            assert st[k] == gst[k] and tst[k] == gst[k], (fmt, k)
        for b in range(B):
            ref, _ = sc.render_tensor(cams[b], W, H, format=fmt, max_level=depth)
            torch.cuda.synchronize()
            assert ref.cpu().numpy().tobytes() == out[b].tobytes(), (name, depth, fmt, b)
    sc.close()


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_render_views_soft_shadows(pkg, scene_data, depth):
    """Sample s of pixel (x, y) of view b draws what the single frame draws: the key is y*W + x, not the batch index."""
    sc = pkg.Scene(scene_data("cornell"))
    W, H, B = 61, 37, 3  # (W*H not a multiple of the tile: views start inside a wave's worth of items)
    cams = _cams(pkg, B, W, H)
    soft = dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(4096, 3), samples=16, seed=11)
    got, gst = sc.render_views(cams, W, H, max_level=depth, **soft)
    singles = [sc.render_soft(cams[b], W, H, max_level=depth, **soft) for b in range(B)]
    for b in range(B):
        assert same_bits(got[b], singles[b][0]), (depth, b)
    for k in STAT_KEYS:
        assert gst[k] == sum(s[1][k] for s in singles), k
    assert gst["soft_shadow_rays"] > 0
    for fmt in FORMATS:
        t, _ = sc.render_views_tensor(cams, W, H, format=fmt, max_level=depth, **soft)
        for b in range(B):
            ref, _ = sc.render_tensor(cams[b], W, H, format=fmt, max_level=depth, **soft)
            torch.cuda.synchronize()
            assert ref.cpu().numpy().tobytes() == t[b].cpu().numpy().tobytes(), (fmt, b)
    # only point lights off, spherical ones on (the reference's soft-shadow-only frame)
    no_point = np.zeros((0, 6), np.float32)
    got, _ = sc.render_views(cams, W, H, lights=no_point, max_level=depth, **soft)
    for b in range(B):
        assert same_bits(got[b], sc.render_soft(cams[b], W, H, lights=no_point, max_level=depth, **soft)[0]), b
    sc.close()


def test_edge_batches(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"))
    W, H = 40, 24
    hit_cams = _cams(pkg, 2, W, H)
    away = hit_cams[0].copy()
    away[0:3] = np.float32([50.0, 60.0, 70.0])  # looking at empty space far from the box: every ray misses
    away2 = away.copy()
    away2[3] += np.float32(0.5)
    mixed = np.ascontiguousarray(np.stack([away, hit_cams[0], away2, hit_cams[1]]))
    got, st = sc.render_views(mixed, W, H, max_level=2)
    for b in range(4):
        assert same_bits(got[b], sc.render(mixed[b], W, H, max_level=2)[0]), b
    assert not got[0].any() and not got[2].any() and got[1].any() and got[3].any()
    # every view misses: black, no shading work at all
    none = np.ascontiguousarray(np.stack([away, away2, away]))
    for fmt in FORMATS:
        out, st = _export_views(pkg, sc, none, W, H, fmt, max_level=2)
        for b in range(3):
            ref, _ = sc.render_tensor(none[b], W, H, format=fmt, max_level=2)
            torch.cuda.synchronize()
            assert ref.cpu().numpy().tobytes() == out[b].tobytes(), (fmt, b)
        assert st["shadow_rays"] == 0 and st["reflection_rays"] == 0 and st["primary_rays"] == 3 * W * H
    hv, _ = _trace_views(pkg, sc, none, W, H)
    assert not hv.view(pkg.HIT_DTYPE)["hit"].any()
    # 64 views of 64x64
    many = _cams(pkg, 64, 64, 64, spread=0.2)
    t, st = sc.render_views_tensor(many, 64, 64, format="rgb", max_level=2)
    torch.cuda.synchronize()
    a = t.cpu().numpy().reshape(64, -1, 3)
    for b in range(64):
        assert same_bits(a[b], sc.render(many[b], 64, 64, max_level=2)[0]), b
    sc.close()


def test_batch_leaves_the_prediction_record_alone(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"))
    W, H = 96, 64
    cam = pkg.scenes.default_camera(W, H)
    first, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == EXACT
    for _ in range(2):
        rgb, _ = sc.render(cam, W, H, max_level=2)
        assert sc.last_render_path() == PREDICTED and rgb.tobytes() == first.tobytes()
    t0, _ = sc.render_tensor(cam, W, H, format="rgba8", max_level=2)
    torch.cuda.synchronize()
    t0 = t0.cpu().numpy()
    assert sc.last_render_path() == PREDICTED
    # batches of the same and of other shapes, depths and light sets in between
    sc.render_views(_cams(pkg, 5, W, H), W, H, max_level=2)
    sc.render_views(_cams(pkg, 2, 33, 17), 33, 17, max_level=4)
    sc.render_views_tensor(_cams(pkg, 3, W, H), W, H, format="chw", max_level=2)
    rgb, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == PREDICTED, "a batch must not touch the scene's prediction record"
    assert rgb.tobytes() == first.tobytes()
    t1, _ = sc.render_tensor(cam, W, H, format="rgba8", max_level=2)
    torch.cuda.synchronize()
    assert sc.last_render_path() == PREDICTED and t1.cpu().numpy().tobytes() == t0.tobytes()
    sc.close()


def test_batch_leaves_frame_hints_alone(pkg):
    pkg.debug_set_hint_thresholds(100, 60)  # (most tiles that reach the tree are hard: the hint lists are busy)
    pkg.set_frame_hints(1)
    try:
        sc = pkg.Scene(pkg.scenes.make_dragon(60_000))
        W, H = 320, 200
        cam = pkg.scenes.default_camera(W, H)
        h0, n0 = _trace_single(pkg, sc, cam, W, H)
        for _ in range(4):  # hinted frames
            h, n = _trace_single(pkg, sc, cam, W, H)
            assert h.tobytes() == h0.tobytes() and n.tobytes() == n0.tobytes()
        counts = sc.hint_counts()
        hv, nv = _trace_views(pkg, sc, _cams(pkg, 3, W, H), W, H)
        sc.render_views(_cams(pkg, 2, W, H), W, H, max_level=2)
        assert sc.hint_counts() == counts, "a batch must not touch the frame hints"
        for _ in range(4):
            h, n = _trace_single(pkg, sc, cam, W, H)
            assert h.tobytes() == h0.tobytes() and n.tobytes() == n0.tobytes()
        sc.close()
    finally:
        pkg.set_frame_hints(-1)
        pkg.debug_set_hint_thresholds(0, 0)


def test_export_is_ordered_behind_the_callers_stream(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"))
    W, H, B = 256, 160, 4
    cams = _cams(pkg, B, W, H)
    ref, _ = sc.render_views(cams, W, H, max_level=2)
    s = torch.cuda.Stream()
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            big = big @ big  # keeps the stream busy
        out.fill_(-7.0)  # enqueued BEFORE the call: the export must land after it
    sc.render_views_tensor(cams, W, H, format="rgb", out=out, stream=s, max_level=2)
    with torch.cuda.stream(s):
        copy = out.clone()  # enqueued AFTER the call: sees the views
    torch.cuda.synchronize()
    assert same_bits(copy.cpu().numpy().reshape(B, -1, 3), ref)
    assert same_bits(out.cpu().numpy().reshape(B, -1, 3), ref)
    # trace: the camera table of an asynchronous call may be reused by the caller at once
    hb, hi, hok = _guarded(B * 64 * 48 * 16)
    tab = _cams(pkg, B, 64, 48)
    want = _trace_views(pkg, sc, tab, 64, 48)[0]
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            big = big @ big
    sc.trace_views_device(tab, 64, 48, hi.data_ptr(), stream=s.cuda_stream)
    tab[:] = 0.0  # (overwritten while the copy may still be queued)
    assert hok() and hi.cpu().numpy().reshape(B, -1).tobytes() == want.tobytes()
    sc.close()


def test_views_match_the_oracle(pkg, orc, scene_data):
    """3 views of 48x32 of Cornell, depth 2, point and spherical lights: every view within 1e-5 of the oracle's ray-list shading of
    that view's row-major rays (ray i = pixel i: the same soft-shadow key), and the stats are the oracle's summed over the views."""
    sd = scene_data("cornell")
    o = orc.OracleScene(sd)
    sc = pkg.Scene(sd)
    W, H, B = 48, 32, 3
    cams = _cams(pkg, B, W, H)
    lights = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    soft = dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(1000, 5), samples=6, seed=123)
    got, gst = sc.render_views(cams, W, H, lights=lights, max_level=2, **soft)
    tot = {k: 0 for k in STAT_KEYS}
    for b in range(B):
        rays = orc.generate_rays(cams[b], W, H)
        want, wc = o.shade_rays(rays, lights, max_level=2, threads=16, **soft)
        assert np.array_equal(np.isnan(got[b]), np.isnan(want)), b
        eq = _same_bits_elementwise(got[b], want)
        with np.errstate(invalid="ignore"):  # (inf - inf where the bits are equal: masked by eq)
            err = np.where(eq, 0.0, np.abs(got[b].astype(np.float64) - want))
        assert not np.isnan(err).any() and float(err.max(initial=0.0)) <= 1e-5, (b, float(np.nanmax(err, initial=0.0)))
        for k in STAT_KEYS:
            tot[k] += wc[k]
    for k in STAT_KEYS:
        assert gst[k] == tot[k], k
    sc.close()
    o.close()

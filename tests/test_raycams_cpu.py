"""No GPU: ray cameras (include/cgrt.h CgrtRayCamera, cgrt_generate_rays_raycam, cgrt_trace_primary_raycams_device,
cgrt_render_raycams_device, cgrt_enqueue_render_raycams_device, cgrt_render_raycams_light_sets_device).

* The struct is 80 bytes; the five entries are exported and bound.
* Each entry checks its arguments before any device work on a host-only scene, in its Trackball twin's order with the camera checks
  where the twin checks `cams`: every bad argument is CGRT_E_ARG, an otherwise valid call CGRT_E_NO_DEVICE.
* Tiles are exact: the rays of tile() in the numpy restatement (tests/raycam_ref.py) are the full frame's region, bit for bit.
* The constructors give hand-computed values and refuse non-finite fields.
* from_trackball is close to the Trackball: the oracle's hit flags on its rays agree with those on oracle.generate_rays on >= 99.5 %
  of the pixels of cornell, monkey and cube at 96x64, and at least 5 % of the pixels hit."""
import ctypes as C

import numpy as np
import pytest

import raycam_ref as R

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_generate_rays_raycam", "cgrt_trace_primary_raycams_device", "cgrt_render_raycams_device",
           "cgrt_enqueue_render_raycams_device", "cgrt_render_raycams_light_sets_device")


def test_struct_and_exports(pkg):
    assert C.sizeof(pkg.RayCamera) == 80
    assert pkg.RayCamera.x_off.offset == 72 and pkg.RayCamera.y_off.offset == 76
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym)


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_OUT = np.zeros(64, np.float32)  # a non-NULL output: every call here fails before anything is written


def _cam_table(pkg, B, edit=None):
    a = np.repeat(pkg.raycam_array(R.pinhole(pkg, 8, 8)), max(B, 1), axis=0)
    a.view(np.int32)[:, 18] = np.arange(len(a)) % 100  # (different offsets per camera)
    a.view(np.int32)[:, 19] = -(np.arange(len(a)) % 100)
    if edit:
        edit(a)
    return a


def _soft(pkg, **bad):
    sph = np.ascontiguousarray(pkg.scenes.CORNELL_SPHERICAL_LIGHTS, np.float32)
    units = pkg.unit_vector_table(64, 0)
    q = dict(spherical=sph.ctypes.data, unit_vectors=units.ctypes.data, nspherical=len(sph), samples=4, nunits=len(units), seed=0,
             closest_hit=0)
    q.update(bad)
    return pkg.SoftShadows(**q), (sph, units)


def _sets(scene, **bad):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    off = np.asarray([0, len(L), len(L)], np.uint32)
    q = dict(nsets=2, lights=L.ctypes.data, light_offsets=off.ctypes.data, spherical=None, spherical_offsets=None)
    q.update(bad)
    import __graft_entry__ as entry

    return entry.load_package().LightSets(**q), (L, off)


def _call(pkg, scene, entry, B=2, W=8, H=8, cams="ok", edit=None, nviews=None, lights="ok", nl=None, soft=None, max_level=2, out="ok", fmt=0,
          handle="ok", aov=None, sets="ok"):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    a = _cam_table(pkg, 1 if entry == "generate" else B, edit)  # (generate takes one camera)
    cp = a.ctypes.data_as(C.c_void_p) if cams == "ok" else None
    n = B if nviews is None else nviews
    d_out = None if out is None else C.c_void_p(_OUT.ctypes.data + (0 if out == "ok" else out))
    h = scene._h if handle == "ok" else None
    lp = None if lights is None else L.ctypes.data_as(C.c_void_p)
    nlights = len(L) if nl is None else nl
    st, t = pkg.RenderStats(), C.c_uint64()
    q = None if soft is None else C.byref(soft)
    av = None if aov is None else C.byref(aov)
    lib = pkg.lib()
    if entry == "generate":
        return lib.cgrt_generate_rays_raycam(h, cp, W, H, d_out)
    if entry == "trace":
        return lib.cgrt_trace_primary_raycams_device(h, cp, n, W, H, d_out, None, None)
    if entry == "render":
        return lib.cgrt_render_raycams_device(h, cp, n, W, H, lp, nlights, q, max_level, d_out, fmt, None, C.byref(st), av)
    if entry == "enqueue":
        return lib.cgrt_enqueue_render_raycams_device(h, cp, n, W, H, lp, nlights, q, max_level, d_out, fmt, None, C.byref(t), av)
    s, keep = _sets(scene) if sets == "ok" else (None, None)
    return lib.cgrt_render_raycams_light_sets_device(h, cp, n, W, H, None if s is None else C.byref(s), q, max_level, d_out, fmt, None, C.byref(st))


def _set(word, value):
    def edit(a):
        a[-1, word] = value  # (the batch's last camera: every camera is checked)

    return edit


def _set_off(word, value):
    def edit(a):
        a.view(np.int32)[-1, word] = value

    return edit


@pytest.mark.parametrize("entry", ["generate", "trace", "render", "enqueue", "sets"])
def test_argument_order(pkg, host_scene, entry):
    err = pkg.lib().cgrt_last_error
    call = lambda **kw: _call(pkg, host_scene, entry, **kw)  # noqa: E731
    assert call() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert b"host-only" in err()
    assert call(B=1) == E_NO_DEVICE
    assert call(handle=None) == E_ARG
    assert call(cams=None) == E_ARG
    assert call(out=None) == E_ARG
    # the camera checks: a non-finite field (every one of the 18), a direction that is identically zero, the offsets
    for word in range(18):
        for v in (np.nan, np.inf, -np.inf):
            assert call(edit=_set(word, v)) == E_ARG, (word, v)
            assert b"non-finite" in err()

    def no_dir(a):
        a[-1, 9:18] = 0.0

    assert call(edit=no_dir) == E_ARG and b"all zero" in err()

    def ortho_like(a):  # dir_dx = dir_dy = 0 with a direction is an orthographic camera: fine
        a[-1, 12:18] = 0.0

    assert call(edit=ortho_like) == E_NO_DEVICE
    lim = 1 << 24
    for word in (18, 19):
        assert call(edit=_set_off(word, lim - 8)) == E_NO_DEVICE, "|off| + size == 2^24 still converts exactly"
        assert call(edit=_set_off(word, -(lim - 8))) == E_NO_DEVICE
        for v in (lim - 7, -(lim - 7), 0x7FFFFFFF, -0x80000000):
            assert call(edit=_set_off(word, v)) == E_ARG, (word, v)
            assert b"2^24" in err()
    # they come where the twin checks `cams`: before the batch's count and size, after the pointer checks
    if entry != "generate":
        assert call(edit=_set(3, np.nan), nviews=2, W=0) == E_ARG and b"non-finite" in err()
        assert call(edit=_set(3, np.nan), out=None) == E_ARG and b"non-finite" not in err()
        assert call(nviews=0) == E_ARG and b"nviews" in err()
        assert call(nviews=2, W=46341, H=23171) == E_ARG and b"0x7fffffff" in err()
        assert call(nviews=1 << 18, B=1 << 18, W=1, H=1) == E_NO_DEVICE, "2^18 super-tiles still fit one launch"
        assert call(nviews=(1 << 18) + 1, B=(1 << 18) + 1, W=1, H=1) == E_ARG and b"super-tiles" in err()
    assert call(W=0) == E_ARG and call(H=-2) == E_ARG
    if entry == "generate":
        return
    if entry == "trace":
        assert call(out=2) == E_ARG, "d_hits not 4-byte aligned"
        return
    for ml in (-1, 17):
        assert call(max_level=ml) == E_ARG
    assert call(max_level=0) == E_NO_DEVICE and call(max_level=16) == E_NO_DEVICE
    for fmt in (0, 1, 2):
        assert call(fmt=fmt) == E_NO_DEVICE
    for fmt in (3, -1):
        assert call(fmt=fmt) == E_ARG and b"format" in err()
    assert call(out=2) == E_ARG and b"aligned" in err()
    assert call(nviews=0, fmt=9) == E_ARG and b"nviews" in err()
    if entry == "sets":
        assert call(sets=None) == E_ARG
        assert call(edit=_set(0, np.inf), W=0) == E_ARG and b"non-finite" in err(), "the cameras are checked with the pointers"
        return
    assert call(lights=None) == E_ARG, "lights missing"
    assert call(lights=None, nl=0) == E_NO_DEVICE
    assert call(lights=None, edit=_set(3, np.nan)) == E_ARG and b"non-finite" not in err(), "lights are checked before the cameras"
    good, keep = _soft(pkg)
    assert call(soft=good) == E_NO_DEVICE
    for bad in (dict(samples=0), dict(nunits=0), dict(spherical=None)):
        q, keep2 = _soft(pkg, **bad)
        assert call(soft=q) == E_ARG, bad
    # aov: NULL is the plain frame; a record without a plane, depth 0 and a misaligned plane are refused as in the twin
    assert call(aov=pkg.AovOut()) == E_ARG
    plane = pkg.AovOut.from_pointers({"depth": _OUT.ctypes.data})
    assert call(aov=plane) == E_NO_DEVICE
    assert call(aov=plane, max_level=0) == E_ARG
    assert call(aov=pkg.AovOut.from_pointers({"depth": _OUT.ctypes.data + 2})) == E_ARG


def test_python_wrappers_on_a_host_scene(pkg, host_scene):
    cam = R.pinhole(pkg, 8, 8)
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.generate_rays_raycam(cam, 8, 8)
    assert e.value.code == E_NO_DEVICE
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.trace_raycams_device([cam, cam.tile(1, 2)], 8, 8, _OUT.ctypes.data)
    assert e.value.code == E_NO_DEVICE
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.render_raycams_device(cam, 8, 8, _OUT.ctypes.data, max_level=17)
    assert e.value.code == E_ARG
    for bad in (np.zeros((2, 9), np.float32), np.zeros((2, 20), np.float64), [cam, 3], [pkg.Camera()]):
        with pytest.raises(ValueError):
            pkg.raycam_array(bad)
    a = pkg.raycam_array([cam, cam.tile(4, -9)])
    assert a.shape == (2, 20) and a.dtype == np.float32 and list(a.view(np.int32)[1, 18:20]) == [4, -9]
    assert pkg.raycam_array(a) is a or np.array_equal(pkg.raycam_array(a).view(np.uint32), a.view(np.uint32))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        host_scene.render_raycams_tensor([cam, cam], 8, 6, out=torch.zeros((3, 6, 8, 3), dtype=torch.float32))
    with pytest.raises(ValueError):
        host_scene.render_raycams_tensor(cam, 8, 6, aovs=("depth",), light_sets=[np.zeros((1, 6), np.float32)])


@pytest.mark.parametrize("kind", ["pinhole", "ortho", "mixed"])
def test_tiles_are_exact_in_the_restatement(pkg, kind):
    W, H = 150, 101
    cam = R.camera_set(pkg, W, H)[kind].tile(-37, 1000)  # (a camera that already carries offsets)
    full = R.rays_of(cam, W, H).reshape(H, W, 7)
    assert np.isfinite(full[..., :6]).all()
    for x0, y0, w, h in ((0, 0, W, H), (64, 0, W - 64, 50), (0, 50, 64, H - 50), (149, 100, 1, 1), (13, 7, 31, 29)):
        tile = R.rays_of(cam.tile(x0, y0), w, h).reshape(h, w, 7)
        assert np.array_equal(tile.view(np.uint32), full[y0 : y0 + h, x0 : x0 + w].view(np.uint32)), (kind, x0, y0)
    t = cam.tile(5, 6).tile(-2, 3)
    assert (t.x_off, t.y_off) == (-37 + 3, 1000 + 9) and (cam.x_off, cam.y_off) == (-37, 1000), "tile() adds up and copies"


def test_from_pinhole_hand_values(pkg):
    # K with skew and non-square pixels; its inverse by hand: [[1/fx, -s/(fx fy), (s cy - cx fy)/(fx fy)], [0, 1/fy, -cy/fy], [0, 0, 1]]
    fx, fy, s, cx, cy = 200.0, 100.0, 10.0, 31.5, 20.25
    K = np.array([[fx, s, cx], [0, fy, cy], [0, 0, 1]])
    dx = np.array([1 / fx, 0, 0])
    dy = np.array([-s / (fx * fy), 1 / fy, 0])
    d0 = np.array([(s * cy - cx * fy) / (fx * fy), -cy / fy, 1.0]) + 0.5 * dx + 0.5 * dy  # pixel centres at +0.5
    c = pkg.RayCamera.from_pinhole(K, np.eye(4))
    assert np.array_equal(np.float32(c.dir[:]), d0.astype(np.float32)) or np.allclose(c.dir[:], d0, rtol=0, atol=1e-7)
    assert np.allclose(c.dir_dx[:], dx, rtol=0, atol=1e-9) and np.allclose(c.dir_dy[:], dy, rtol=0, atol=1e-9)
    assert list(c.origin) == [0, 0, 0] and not any(c.origin_dx) and not any(c.origin_dy) and (c.x_off, c.y_off) == (0, 0)
    # a pose: rotate 90 degrees about y (camera z -> world x, camera x -> world -z), translate
    P = np.array([[0, 0, 1, 4.0], [0, 1, 0, 5.0], [-1, 0, 0, 6.0]])
    c = pkg.RayCamera.from_pinhole(K, P)
    assert list(c.origin) == [4, 5, 6]
    assert np.allclose(c.dir[:], [d0[2], d0[1], -d0[0]], rtol=0, atol=1e-7)
    assert np.allclose(c.dir_dx[:], [0, 0, -1 / fx], rtol=0, atol=1e-9) and np.allclose(c.dir_dy[:], [0, 1 / fy, s / (fx * fy)], rtol=0, atol=1e-9)
    # OpenGL axes: the same K, camera y up and z backward -> y and z of the camera-space direction change sign
    g = pkg.RayCamera.from_pinhole(K, np.eye(4), convention="opengl")
    assert np.allclose(g.dir[:], d0 * [1, -1, -1], rtol=0, atol=1e-7)
    assert np.allclose(g.dir_dx[:], dx * [1, -1, -1], rtol=0, atol=1e-9) and np.allclose(g.dir_dy[:], dy * [1, -1, -1], rtol=0, atol=1e-9)
    # the centre pixel of a centred K looks straight down the axis: +z (opencv), -z (opengl)
    Kc = np.array([[50.0, 0, 4.5], [0, 50.0, 3.5], [0, 0, 1]])
    for conv, z in (("opencv", 1.0), ("opengl", -1.0)):
        r = R.rays_of(pkg.RayCamera.from_pinhole(Kc, np.eye(4), convention=conv), 9, 7).reshape(7, 9, 7)
        assert np.array_equal(r[3, 4, 3:6], np.float32([0, 0, z]))
    with pytest.raises(ValueError):
        pkg.RayCamera.from_pinhole(K, np.eye(4), convention="blender")
    with pytest.raises(ValueError):
        pkg.RayCamera.from_pinhole(np.eye(4), np.eye(4))


def test_orthographic_hand_values(pkg):
    c = pkg.RayCamera.orthographic(origin=(1, 2, 3), right=(1, 0, 0), up=(0, 0, 1), forward=(0, -1, 0), pixel_size=0.5)
    assert list(c.origin) == [1.25, 2, 3.25] and list(c.origin_dx) == [0.5, 0, 0] and list(c.origin_dy) == [0, 0, 0.5]
    assert list(c.dir) == [0, -1, 0] and not any(c.dir_dx) and not any(c.dir_dy)
    r = R.rays_of(c, 4, 3).reshape(3, 4, 7)
    assert np.array_equal(r[2, 3, :6], np.float32([1.25 + 1.5, 2, 3.25 + 1.0, 0, -1, 0]))
    c = pkg.RayCamera.orthographic((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 2), pixel_size=(0.25, 2.0))
    assert list(c.origin) == [0.125, 1, 0] and list(c.origin_dx) == [0.25, 0, 0] and list(c.origin_dy) == [0, 2, 0]
    assert np.array_equal(R.rays_of(c, 2, 2)[:, 3:6], np.float32([[0, 0, 1]] * 4)), "the direction is normalised per ray"


def test_non_finite_fields_are_refused(pkg):
    K = np.array([[100.0, 0, 4], [0, 100.0, 4], [0, 0, 1]])
    P = np.eye(4)
    P[0, 3] = np.nan
    with pytest.raises(ValueError):
        pkg.RayCamera.from_pinhole(K, P)
    with pytest.raises(ValueError):
        pkg.RayCamera.orthographic((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, np.inf), 1.0)
    with pytest.raises(ValueError):
        pkg.RayCamera.orthographic((0, 0, 0), (1e39, 0, 0), (0, 1, 0), (0, 0, 1), 1.0)  # (finite in float64, not in float32)
    with pytest.raises(ValueError):
        pkg.RayCamera.from_fields((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, np.nan, 1), (0, 0, 0), (0, 0, 0))


@pytest.mark.parametrize("name", ["cornell", "monkey", "cube"])
def test_from_trackball_is_close_to_the_trackball(pkg, orc, scene_data, name):
    W, H = 96, 64
    cam = pkg.scenes.default_camera(W, H)
    o = orc.OracleScene(scene_data(name))
    mine = R.rays_of(pkg.RayCamera.from_trackball(cam, W, H), W, H)
    ref = orc.generate_rays(cam, W, H)
    a, b = o.intersect(mine), o.intersect(ref)
    o.close()
    agree = float((a["hit"] == b["hit"]).mean())
    frac = float(b["hit"].mean())
    print(name, "direction error", float(np.abs(mine[:, 3:6] - ref[:, 3:6]).max()), "flags agree", agree, "hit fraction", frac)
    assert agree >= 0.995
    assert frac >= 0.05 and float(a["hit"].mean()) >= 0.05
    assert np.array_equal(mine[:, 6], ref[:, 6])
    c2 = pkg.RayCamera.from_trackball(pkg.Camera.from_array(cam), W, H)
    assert bytes(c2) == bytes(pkg.RayCamera.from_trackball(cam, W, H))

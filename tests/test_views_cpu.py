"""No GPU: multi-view frames (include/cgrt.h cgrt_trace_primary_views_device, cgrt_render_views, cgrt_render_views_device).

* The three entries are exported and bound.
* Each checks its arguments before any device work, in the documented order, on a host-only scene: every bad argument is CGRT_E_ARG
  (NULL scene / cams / output, nlights without lights, nviews == 0, W or H <= 0, nviews*W*H > 0x7fffffff, max_level, soft, format,
  alignment), an otherwise valid call CGRT_E_NO_DEVICE.
* camera_array takes a (B, 9) array or a sequence of Camera, and Scene.render_views_tensor refuses a wrong `out` with ValueError
  before any call."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_trace_primary_views_device", "cgrt_render_views", "cgrt_render_views_device")


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym)


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_OUT = np.zeros(64, np.float32)  # a non-NULL output: every call here fails before anything is written


def _cams(pkg, B, W=8, H=8):
    a = np.repeat(pkg.scenes.default_camera(W, H)[None, :], max(B, 1), axis=0).astype(np.float32)
    a[:, 4] += np.arange(len(a), dtype=np.float32) * np.float32(0.1)
    return np.ascontiguousarray(a)


def _soft(pkg, **bad):
    sph = np.ascontiguousarray(pkg.scenes.CORNELL_SPHERICAL_LIGHTS, np.float32)
    units = pkg.unit_vector_table(64, 0)
    q = dict(spherical=sph.ctypes.data, unit_vectors=units.ctypes.data, nspherical=len(sph), samples=4, nunits=len(units), seed=0,
             closest_hit=0)
    q.update(bad)
    return pkg.SoftShadows(**q), (sph, units)


def _call(pkg, scene, entry, B=2, W=8, H=8, cams="ok", nviews=None, lights="ok", nl=None, soft=None, max_level=2, out="ok", fmt=0,
          handle="ok", normals=None):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    a = _cams(pkg, B)
    cp = a.ctypes.data_as(C.c_void_p) if cams == "ok" else None
    n = B if nviews is None else nviews
    d_out = None if out is None else C.c_void_p(_OUT.ctypes.data + (0 if out == "ok" else out))
    h = scene._h if handle == "ok" else None
    lp = None if lights is None else L.ctypes.data_as(C.c_void_p)
    nlights = len(L) if nl is None else nl
    st = pkg.RenderStats()
    q = None if soft is None else C.byref(soft)
    lib = pkg.lib()
    if entry == "trace":
        return lib.cgrt_trace_primary_views_device(h, cp, n, W, H, d_out, normals, None)
    if entry == "render":
        return lib.cgrt_render_views(h, cp, n, W, H, lp, nlights, q, max_level, d_out, C.byref(st))
    return lib.cgrt_render_views_device(h, cp, n, W, H, lp, nlights, q, max_level, d_out, fmt, None, C.byref(st))


@pytest.mark.parametrize("entry", ["trace", "render", "device"])
def test_argument_order(pkg, host_scene, entry):
    err = pkg.lib().cgrt_last_error
    assert _call(pkg, host_scene, entry) == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert b"host-only" in err()
    assert _call(pkg, host_scene, entry, B=1) == E_NO_DEVICE
    assert _call(pkg, host_scene, entry, handle=None) == E_ARG
    assert _call(pkg, host_scene, entry, cams=None) == E_ARG
    assert b"cams" in err()
    assert _call(pkg, host_scene, entry, out=None) == E_ARG
    assert _call(pkg, host_scene, entry, nviews=0) == E_ARG
    assert b"nviews" in err()
    assert _call(pkg, host_scene, entry, W=0) == E_ARG and _call(pkg, host_scene, entry, H=-2) == E_ARG
    # nviews * W * H: 0x7fffffff is the last size that passes the check (with 1x1 views it is the super-tile limit that refuses it)
    assert _call(pkg, host_scene, entry, nviews=2, W=46341, H=23171) == E_ARG  # 2 * 46341 * 23171 = 0x80000006
    assert b"0x7fffffff" in err()
    assert _call(pkg, host_scene, entry, nviews=0xFFFFFFFF, W=1, H=1) == E_ARG
    assert b"0x7fffffff" in err()
    assert _call(pkg, host_scene, entry, nviews=0x80000000, W=1, H=1) == E_ARG
    assert _call(pkg, host_scene, entry, nviews=1 << 18, W=1, H=1) == E_NO_DEVICE, "2^18 super-tiles still fit one launch"
    assert _call(pkg, host_scene, entry, nviews=(1 << 18) + 1, W=1, H=1) == E_ARG
    assert b"super-tiles" in err()
    # (the pointer checks come first: a NULL output with a bad count is a NULL argument)
    assert _call(pkg, host_scene, entry, out=None, nviews=0) == E_ARG
    if entry == "trace":
        assert _call(pkg, host_scene, entry, out=2) == E_ARG, "d_hits not 4-byte aligned"
        return
    assert _call(pkg, host_scene, entry, lights=None) == E_ARG, "lights missing"
    assert _call(pkg, host_scene, entry, lights=None, nl=0) == E_NO_DEVICE, "no lights at all is a valid batch"
    for ml in (-1, 17):
        assert _call(pkg, host_scene, entry, max_level=ml) == E_ARG
    assert _call(pkg, host_scene, entry, max_level=0) == E_NO_DEVICE and _call(pkg, host_scene, entry, max_level=16) == E_NO_DEVICE
    good, keep = _soft(pkg)
    assert _call(pkg, host_scene, entry, soft=good) == E_NO_DEVICE
    for bad in (dict(samples=0), dict(samples=(1 << 24) + 1), dict(nunits=0), dict(spherical=None), dict(unit_vectors=None)):
        q, keep2 = _soft(pkg, **bad)
        assert _call(pkg, host_scene, entry, soft=q) == E_ARG, bad
    if entry == "device":
        for fmt in (0, 1, 2):
            assert _call(pkg, host_scene, entry, fmt=fmt) == E_NO_DEVICE
        for fmt in (3, -1, 7):
            assert _call(pkg, host_scene, entry, fmt=fmt) == E_ARG, fmt
            assert b"format" in err()
        assert _call(pkg, host_scene, entry, out=2) == E_ARG, "d_out not 4-byte aligned"
        assert b"aligned" in err()
        # order: a bad size is reported before a bad format
        assert _call(pkg, host_scene, entry, nviews=0, fmt=9) == E_ARG and b"nviews" in err()
        assert _call(pkg, host_scene, entry, max_level=99, fmt=9) == E_ARG and b"depth" in err()


def test_camera_array(pkg):
    a = np.arange(27, dtype=np.float32).reshape(3, 9)
    assert np.array_equal(pkg.camera_array(a), a)
    cams = [pkg.Camera.from_array(r) for r in a]
    assert np.array_equal(pkg.camera_array(cams), a)
    assert pkg.camera_array(a.tolist()).dtype == np.float32
    for bad in (np.zeros(9, np.float32), np.zeros((2, 8), np.float32), np.zeros((2, 3, 9), np.float32)):
        with pytest.raises(ValueError):
            pkg.camera_array(bad)


def test_render_views_tensor_rejects_out_before_any_call(pkg, host_scene):
    torch = pytest.importorskip("torch")
    cams = _cams(pkg, 3)
    W, H = 8, 6

    def rejects(out, fmt="rgb"):
        with pytest.raises(ValueError):
            host_scene.render_views_tensor(cams, W, H, format=fmt, out=out)

    rejects(torch.zeros((3, H, W, 3), dtype=torch.float64))  # dtype
    rejects(torch.zeros((3, H, W, 3), dtype=torch.uint8))
    rejects(torch.zeros((3, H, W, 4), dtype=torch.float32), "rgba8")
    rejects(torch.zeros((2, H, W, 3), dtype=torch.float32))  # shape: B
    rejects(torch.zeros((3, W, H, 3), dtype=torch.float32))
    rejects(torch.zeros((H, W, 3), dtype=torch.float32))
    rejects(torch.zeros((3, H, W, 3), dtype=torch.float32), "chw")
    rejects(torch.zeros((3, 3, H, W), dtype=torch.float32), "rgb")
    rejects(torch.zeros((3, H, W, 3), dtype=torch.uint8), "rgba8")
    rejects(torch.zeros((3, H, W, 3), dtype=torch.float32).transpose(1, 2).contiguous().transpose(1, 2))  # non-contiguous
    rejects(torch.zeros((3, 3, W, H), dtype=torch.float32).transpose(2, 3), "chw")
    rejects(torch.zeros((6, H, W, 4), dtype=torch.uint8)[::2], "rgba8")
    rejects(np.zeros((3, H, W, 3), np.float32))  # not a tensor
    rejects(torch.zeros((3, H, W, 3), dtype=torch.float32), "bgr")  # unknown format
    # a valid `out` on the CPU is refused too (the scene's device), and a host-only scene with no `out` at all
    rejects(torch.zeros((3, H, W, 3), dtype=torch.float32))
    rejects(None)

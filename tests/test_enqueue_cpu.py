"""No GPU: enqueued frames (include/cgrt.h cgrt_enqueue_*).

* The four symbols are exported.
* On a host-only scene every bad argument of the three enqueue entries is CGRT_E_ARG, in the blocking counterpart's order, and an otherwise
  valid call is CGRT_E_NO_DEVICE; cgrt_enqueue_stats checks its scene.
* The Python methods reject bad tensors before any call.
* The committed resource-usage report shows every existing kernel instantiation unchanged and lists the new ones (their scratch is
  recorded there, not checked: DESIGN.md section 5.14).
* The cap diagnostic (cgrt_debug_strided_waves) reports the default cap."""
import ctypes as C
import os

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("cgrt_enqueue_render_device", "cgrt_enqueue_render_views_device", "cgrt_enqueue_shade_rays_device", "cgrt_enqueue_stats",
        "cgrt_debug_strided_waves")


def test_symbols_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in SYMS:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_OUT = np.zeros(64, np.float32)


def _frame(pkg, scene, enqueue, W=8, H=8, lights="ok", nl=None, soft=None, max_level=2, aa=0, rank=0, nranks=1, out="ok", fmt=0, row_bytes=0,
           cam="ok", handle="ok"):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    c = pkg.Camera.from_array(pkg.scenes.default_camera(max(W, 1), max(H, 1)))
    d_out = C.c_void_p(_OUT.ctypes.data) if out == "ok" else (None if out is None else C.c_void_p(_OUT.ctypes.data + out))
    args = (scene._h if handle == "ok" else None, C.byref(c) if cam == "ok" else None, W, H,
            None if lights is None else L.ctypes.data_as(C.c_void_p), len(L) if nl is None else nl, soft, max_level, aa, rank, nranks, d_out, fmt,
            row_bytes, None)
    if enqueue:
        return pkg.lib().cgrt_enqueue_render_device(*args, C.byref(C.c_uint64()))
    return pkg.lib().cgrt_render_device(*args, C.byref(pkg.RenderStats()))


FRAME_CASES = [dict(), dict(handle=None), dict(cam=None), dict(out=None), dict(lights=None), dict(lights=None, nl=0), dict(W=0), dict(H=-3),
               dict(max_level=-1), dict(max_level=17), dict(max_level=16), dict(rank=1, nranks=1), dict(rank=-1, nranks=2), dict(nranks=0),
               dict(rank=1, nranks=2), dict(fmt=3), dict(fmt=2), dict(row_bytes=92), dict(row_bytes=98), dict(row_bytes=96), dict(out=2),
               dict(W=23171, H=23171), dict(cam=None, out=None, W=0), dict(W=0, max_level=17), dict(max_level=17, rank=3), dict(rank=3, fmt=9),
               dict(fmt=9, out=2)]


def test_frame_entry_checks_like_the_blocking_one(pkg, host_scene):
    for aa in (0, 1):
        for case in FRAME_CASES:
            want = _frame(pkg, host_scene, False, aa=aa, **case)
            got = _frame(pkg, host_scene, True, aa=aa, **case)
            msg_want = pkg.lib().cgrt_last_error()
            assert got == want, (aa, case)
            if want == E_ARG:
                _frame(pkg, host_scene, False, aa=aa, **case)
                assert pkg.lib().cgrt_last_error() == msg_want, (aa, case)
        assert _frame(pkg, host_scene, True, aa=aa) == E_NO_DEVICE
    # NULL ticket is allowed: still the device check
    c = pkg.Camera.from_array(pkg.scenes.default_camera(8, 8))
    assert pkg.lib().cgrt_enqueue_render_device(host_scene._h, C.byref(c), 8, 8, None, 0, None, 2, 0, 0, 1, C.c_void_p(_OUT.ctypes.data), 0, 0, None,
                                                 None) == E_NO_DEVICE


def test_frame_entry_checks_soft_shadows(pkg, host_scene):
    sph = np.zeros((1, 7), np.float32)
    units = np.zeros((4, 3), np.float32)

    def soft(spherical=True, units_=True, samples=16, nunits=4):
        return C.byref(pkg.SoftShadows(sph.ctypes.data if spherical else None, units.ctypes.data if units_ else None, 1, samples, nunits, 0, 0))

    for aa in (0, 1):
        for kw, want in ((dict(), E_NO_DEVICE), (dict(spherical=False), E_ARG), (dict(units_=False), E_ARG), (dict(nunits=0), E_ARG),
                         (dict(samples=0), E_ARG), (dict(samples=(1 << 24) + 1), E_ARG)):
            assert _frame(pkg, host_scene, True, aa=aa, soft=soft(**kw)) == want, (aa, kw)


def _views(pkg, scene, enqueue, cams="ok", nviews=2, W=8, H=8, lights="ok", nl=None, max_level=2, out="ok", fmt=0, handle="ok"):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    a = pkg.camera_array([pkg.scenes.default_camera(8, 8)] * 2)
    args = (scene._h if handle == "ok" else None, a.ctypes.data_as(C.c_void_p) if cams == "ok" else None, nviews, W, H,
            None if lights is None else L.ctypes.data_as(C.c_void_p), len(L) if nl is None else nl, None, max_level,
            C.c_void_p(_OUT.ctypes.data + (0 if out == "ok" else out)) if out is not None else None, fmt, None)
    if enqueue:
        return pkg.lib().cgrt_enqueue_render_views_device(*args, C.byref(C.c_uint64()))
    return pkg.lib().cgrt_render_views_device(*args, C.byref(pkg.RenderStats()))


def test_views_entry_checks_like_the_blocking_one(pkg, host_scene):
    for case in (dict(), dict(handle=None), dict(cams=None), dict(out=None), dict(lights=None), dict(lights=None, nl=0), dict(nviews=0), dict(W=0),
                 dict(H=-1), dict(max_level=17), dict(max_level=-1), dict(fmt=5), dict(out=2), dict(nviews=0, max_level=17), dict(W=0, fmt=5)):
        want = _views(pkg, host_scene, False, **case)
        assert _views(pkg, host_scene, True, **case) == want, case
    assert _views(pkg, host_scene, True) == E_NO_DEVICE


def _rays(pkg, scene, enqueue, n=4, rays="ok", lights="ok", nl=None, max_level=2, rgb="ok", handle="ok"):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    r = np.zeros((8, 7), np.float32)
    args = (scene._h if handle == "ok" else None, r.ctypes.data_as(C.c_void_p) if rays == "ok" else None, n,
            None if lights is None else L.ctypes.data_as(C.c_void_p), len(L) if nl is None else nl, None, max_level,
            C.c_void_p(_OUT.ctypes.data) if rgb == "ok" else None, None)
    if enqueue:
        return pkg.lib().cgrt_enqueue_shade_rays_device(*args, C.byref(C.c_uint64()))
    return pkg.lib().cgrt_shade_rays_device(*args, C.byref(pkg.RenderStats()))


def test_shade_rays_entry_checks_like_the_blocking_one(pkg, host_scene):
    for case in (dict(), dict(handle=None), dict(rays=None), dict(rays=None, n=0), dict(rgb=None), dict(lights=None), dict(lights=None, nl=0),
                 dict(n=0x80000000), dict(max_level=17), dict(max_level=-1), dict(n=0), dict(rgb=None, max_level=17)):
        want = _rays(pkg, host_scene, False, **case)
        assert _rays(pkg, host_scene, True, **case) == want, case
    assert _rays(pkg, host_scene, True) == E_NO_DEVICE


def test_stats_checks_its_scene(pkg, host_scene):
    st = pkg.RenderStats()
    assert pkg.lib().cgrt_enqueue_stats(None, 1, C.byref(st)) == E_ARG
    assert pkg.lib().cgrt_enqueue_stats(host_scene._h, 1, C.byref(st)) == E_NO_DEVICE


def test_python_methods_reject_bad_tensors(pkg, host_scene):
    torch = pytest.importorskip("torch")
    W, H = 8, 6
    cam = pkg.scenes.default_camera(W, H)
    for fmt, shape, dtype in (("rgb", (H, W, 3), torch.float32), ("chw", (3, H, W), torch.float32), ("rgba8", (H, W, 4), torch.uint8)):
        with pytest.raises(ValueError, match="cuda"):
            host_scene.enqueue_render_tensor(cam, W, H, format=fmt, out=torch.zeros(shape, dtype=dtype))
        with pytest.raises(ValueError, match="dtype"):
            host_scene.enqueue_render_tensor(cam, W, H, format=fmt, out=torch.zeros(shape, dtype=torch.float64))
        with pytest.raises(ValueError, match="shape"):
            host_scene.enqueue_render_tensor(cam, W, H, format=fmt, out=torch.zeros((H + 1,) + tuple(shape[1:]), dtype=dtype))
    with pytest.raises(ValueError, match="format"):
        host_scene.enqueue_render_tensor(cam, W, H, format="bgr")
    with pytest.raises(ValueError, match="host-only"):
        host_scene.enqueue_render_tensor(cam, W, H)
    cams = np.stack([cam, cam])
    with pytest.raises(ValueError, match="shape"):
        host_scene.enqueue_render_views_tensor(cams, W, H, out=torch.zeros((3, H, W, 3)))
    with pytest.raises(ValueError, match="cuda"):
        host_scene.enqueue_render_views_tensor(cams, W, H, out=torch.zeros((2, H, W, 3)))
    with pytest.raises(ValueError, match="format"):
        host_scene.enqueue_render_views_tensor(cams, W, H, format="bgr")
    with pytest.raises(ValueError, match="host-only"):
        host_scene.enqueue_shade_rays_tensor(torch.zeros((4, 7)))
    with pytest.raises(ValueError):
        host_scene.enqueue_render_tensor(cam, W, H, out=np.zeros((H, W, 3), np.float32))


def test_resource_usage_report(pkg):
    """profiles/enqueue_resource_usage.txt (tools/enqueue_resource_usage.py): existing instantiations unchanged, new ones listed"""
    with open(os.path.join(ROOT, "profiles", "enqueue_resource_usage.txt")) as f:
        text = f.read()
    assert "# existing instantiations changed: 0" in text
    rows = [ln for ln in text.splitlines() if not ln.startswith("#")]
    assert not [r for r in rows if " existing " in r and " same " not in r]
    new = [r for r in rows if " new " in r]
    for k in ("k_spawn_strided", "k_shade_strided", "k_fold_strided", "k_write_rgb_strided", "k_soft_shadow_strided", "k_trace_pair<true, true>",
              "k_trace_batch<false, true, false, true>", "k_trace_shadow<false, true, false, true>"):
        assert any(k in r for r in new), k


def test_default_cap(pkg):
    if "CGRT_STRIDED_WAVES" in os.environ:
        pytest.skip("the cap is overridden in this environment")
    assert pkg.lib().cgrt_debug_strided_waves() == 6144

"""No GPU: gradients of the surface attributes back to the per-vertex table (cgrt_interpolate_hits_grad*, cgrt_surface_*_grad_device;
include/cgrt.h).

* The four entries are exported and the Scene methods exist.
* On a host-only scene every argument check comes in the forward twin's order with CGRT_E_ARG, and an otherwise valid call gives
  CGRT_E_NO_DEVICE.  n == 0 with NULL arrays passes every argument check (on a host-only scene the answer is then CGRT_E_NO_DEVICE, as
  the forward's; that it succeeds and touches nothing on a device scene is tests/test_surface_grad_gpu.py's).
* tests/surface_grad_ref.py, the float64 restatement the GPU tests hold the device to, is the adjoint of surface_ref.mix:
  <mix(attr), g> == <attr, grad> to the derived bound."""
import ctypes as C

import numpy as np
import pytest

import surface_grad_ref as gr
import surface_ref as sr

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_interpolate_hits_grad", "cgrt_interpolate_hits_grad_device", "cgrt_surface_views_grad_device",
           "cgrt_surface_raycams_grad_device")


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in ("interpolate_hits_grad", "interpolate_hits_grad_device", "surface_views_grad_device", "interpolate_hits_grad_tensor",
                 "surface_views_grad_tensor", "surface_raycams_grad_tensor"):
        assert callable(getattr(pkg.Scene, name, None)), name


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_RAYS = np.zeros((16, 7), np.float32)
_HITS = np.zeros((16, 4), np.uint32)
_TABLE = np.zeros((64, 256), np.float32)
_GOUT = np.zeros(16 * 16 * 2 * 4 + 4, np.float32)
_PLANE = np.zeros(16 * 16 * 2, np.float32)


def _at(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _list(pkg, sc, device, handle="ok", rays=0, hits=0, n=16, gout=0, channels=3, table=0):
    """rays / hits / gout / table: a byte offset into the module's arrays, or None for NULL."""
    p = lambda a, off: None if off is None else _at(a, off)  # noqa: E731
    args = [sc._h if handle == "ok" else None, p(_RAYS, rays), p(_HITS, hits), n, p(_GOUT, gout), channels, p(_TABLE, table)]
    L = pkg.lib()
    return L.cgrt_interpolate_hits_grad_device(*args, None) if device else L.cgrt_interpolate_hits_grad(*args)


@pytest.mark.parametrize("device", [False, True])
def test_list_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _list(pkg, host_scene, device, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(n=0) == E_NO_DEVICE and c(n=0x7fffffff, channels=1) == E_NO_DEVICE
    # rule 1: NULL scene, or with n > 0 NULL rays / hits / grad_out / grad_attr
    assert c(handle=None) == E_ARG
    assert c(rays=None) == E_ARG and c(hits=None) == E_ARG and c(gout=None) == E_ARG and c(table=None) == E_ARG
    assert "NULL" in _err(pkg)
    assert c(rays=None, hits=None, gout=None, table=None, n=0) == E_NO_DEVICE, "NULL arrays with n == 0 pass the argument checks"
    # rule 2: n > 0x7fffffff
    assert c(n=0x80000000) == E_ARG and "0x7fffffff" in _err(pkg)
    # rule 3: channels in 1..256, grad_out within 2^40 bytes
    assert c(channels=0) == E_ARG and "channels" in _err(pkg)
    assert c(channels=257) == E_ARG and "channels" in _err(pkg)
    assert c(channels=1) == E_NO_DEVICE and c(channels=256) == E_NO_DEVICE
    assert c(n=1 << 30, channels=256) == E_NO_DEVICE, "exactly 2^40 bytes"
    assert c(n=(1 << 30) + 1, channels=256) == E_ARG and "2^40" in _err(pkg)
    # rule 4 (device form): every pointer 4-byte aligned
    for kw in ({"rays": 2}, {"hits": 2}, {"gout": 2}, {"table": 2}):
        assert c(**kw) == (E_ARG if device else E_NO_DEVICE), kw
        assert not device or "aligned" in _err(pkg)
    # the order
    assert c(handle=None, n=1 << 40, channels=0, rays=2) == E_ARG and "NULL" in _err(pkg)
    assert c(gout=None, n=1 << 40, channels=0, rays=2) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 40, channels=0, rays=2) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(channels=0, rays=2) == E_ARG and "channels" in _err(pkg)
    assert c(n=(1 << 30) + 1, channels=256, rays=2) == E_ARG and "2^40" in _err(pkg)


def _frames(pkg, sc, raycams, handle="ok", cams="ok", nviews=2, W=16, H=16, depth=0, prim=0, gout=0, channels=3, chw=0, table=0, cam_edit=None):
    if raycams:
        a = pkg.raycam_array([pkg.RayCamera.from_trackball(pkg.scenes.default_camera(16, 16), 16, 16)] * max(nviews, 1))
        if cam_edit:
            a = a.copy()
            cam_edit(a)
    else:
        a = pkg.camera_array(np.stack([pkg.scenes.default_camera(16, 16)] * max(nviews, 1)))
    p = lambda arr, off: None if off is None else _at(arr, off)  # noqa: E731
    f = pkg.lib().cgrt_surface_raycams_grad_device if raycams else pkg.lib().cgrt_surface_views_grad_device
    return f(sc._h if handle == "ok" else None, _at(a) if cams == "ok" else None, nviews, W, H, p(_PLANE, depth), p(_PLANE, prim), p(_GOUT, gout),
             channels, chw, p(_TABLE, table), None)


@pytest.mark.parametrize("raycams", [False, True])
def test_frame_argument_checks_and_their_order(pkg, host_scene, raycams):
    c = lambda **kw: _frames(pkg, host_scene, raycams, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE and c(chw=1) == E_NO_DEVICE
    # rule 1: NULL scene / planes / grad_out / grad_attr
    assert c(handle=None) == E_ARG and c(depth=None) == E_ARG and c(prim=None) == E_ARG
    assert c(gout=None) == E_ARG and "NULL" in _err(pkg)
    assert c(table=None) == E_ARG and "NULL" in _err(pkg)
    # rule 2: the cameras and the views limits, as the forward checks them
    assert c(cams=None) == E_ARG and "cams" in _err(pkg)
    assert c(nviews=0) == E_ARG and c(W=0) == E_ARG and c(H=-1) == E_ARG
    assert c(nviews=3, W=1 << 15, H=1 << 15) == E_ARG and "0x7fffffff" in _err(pkg)
    if raycams:
        def nan_origin(a):
            a.view(np.float32).reshape(len(a), -1)[0, 0] = np.nan

        assert c(cam_edit=nan_origin) == E_ARG and "non-finite" in _err(pkg)
    # rule 3: channels
    assert c(channels=0) == E_ARG and c(channels=257) == E_ARG and "channels" in _err(pkg)
    assert c(channels=1) == E_NO_DEVICE and c(channels=256) == E_NO_DEVICE
    assert c(nviews=1, W=1 << 15, H=1 << 15, channels=256) == E_NO_DEVICE, "the largest frame there is: exactly 2^40 bytes"
    # rule 4: alignment
    for kw in ({"depth": 2}, {"prim": 2}, {"gout": 2}, {"table": 2}):
        assert c(**kw) == E_ARG and "aligned" in _err(pkg), kw
    # the order
    assert c(depth=None, cams=None, channels=0, gout=2) == E_ARG and "NULL argument" in _err(pkg)
    assert c(cams=None, channels=0, gout=2) == E_ARG and "cams" in _err(pkg)
    assert c(W=0, channels=0, gout=2) == E_ARG and "frame size" in _err(pkg)
    assert c(channels=0, gout=2) == E_ARG and "channels" in _err(pkg)


def test_numpy_form_checks_its_arrays(pkg, host_scene):
    rays, hits = np.zeros((4, 7), np.float32), np.zeros(4, pkg.HIT_DTYPE)
    nverts = len(np.asarray(host_scene.sd.pos_nrm).reshape(-1, 6))
    with pytest.raises(ValueError):
        host_scene.interpolate_hits_grad(rays, hits, np.zeros((3, 2), np.float32))  # (not one row per ray)
    with pytest.raises(ValueError):
        host_scene.interpolate_hits_grad(rays, hits, np.zeros((4, 2), np.float32), grad_attr=np.zeros((nverts, 3), np.float32))
    with pytest.raises(ValueError):
        host_scene.interpolate_hits_grad(rays, hits, np.zeros((4, 2), np.float32), grad_attr=np.zeros((nverts, 2), np.float64))
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.interpolate_hits_grad(rays, hits, np.zeros((4, 2), np.float32))
    assert e.value.code == E_NO_DEVICE


@pytest.mark.parametrize("name,C", [("blob", 3), ("monkey", 5), ("cornell", 32)])
def test_restatement_is_the_adjoint_of_the_mix(pkg, orc, scene_data, name, C):
    """<mix(attr), g> == <attr, grad> for the float64 restatement (zero initial table): both sides are the same sum of w * attr * g, the
    left one through surface_ref.mix's float32 mix.  Per item and channel the float32 mix (three rounded products, two rounded sums)
    is within gamma(3) * sum_k |w_k attr_k| of the exact mix, so the two sides differ by at most gamma(3) * sum |w attr g| (plus
    float64 noise far below it)."""
    sd = scene_data(name)
    rays = sr.random_rays(sd, 3000, 5)
    o = orc.OracleScene(sd)
    h = o.intersect(rays)
    o.close()
    prim, hit = h["prim"].copy(), h["hit"].copy()
    prim[::7] = sd.ntris + 3  # out-of-range ids, and a NaN gradient behind every invalid item
    w = sr.weights(sd, rays, h["t"], prim, hit)
    ok = sr.triangle_mask(sd, hit, prim)
    assert ok.sum() >= 500 and (~ok).sum() >= 400
    rng = np.random.default_rng(C)
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    sign = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)  # noqa: E731
    attr = (sign((nverts, C)) * 2.0 ** rng.uniform(-10, 10, (nverts, C))).astype(np.float32)
    g = (sign((len(rays), C)) * 2.0 ** rng.uniform(-10, 10, (len(rays), C))).astype(np.float32)
    g[~ok] = np.nan
    ref, S, m = gr.adjoint(sd, w, prim, hit, g)
    assert np.isfinite(ref).all() and not ref[m == 0].any() and int(m.sum()) == 3 * int(ok.sum())
    mixed = sr.mix(sd, w, prim, hit, attr).astype(np.float64)
    left = float((mixed[ok] * g[ok].astype(np.float64)).sum())
    right = float((attr.astype(np.float64) * ref).sum())
    scale = float((np.abs(attr.astype(np.float64)) * S).sum())  # sum |w attr g|
    print(name, C, "left", left, "right", right, "|diff|", abs(left - right), "allowed", float(gr.gamma(3)) * scale)
    assert abs(left - right) <= float(gr.gamma(3)) * scale

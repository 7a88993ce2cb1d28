"""No GPU: getFinalColor of caller-supplied rays (cgrt_shade_rays / cgrt_shade_rays_device, include/cgrt.h).

* Both entries and the mirror's cgrt_host_shade_rays are exported.
* Every argument is checked before any device work, in the documented order, on a host-only scene: each rule is CGRT_E_ARG and
  wins over the ones after it; an otherwise valid call is CGRT_E_NO_DEVICE.
* Scene.shade_rays_tensor validates its tensors before any call."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2


def test_new_symbols_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ("cgrt_shade_rays", "cgrt_shade_rays_device"):
        assert sym in pkg.EXPORTS and hasattr(L, sym)
    assert hasattr(C.CDLL(pkg.HOST_LIB_PATH), "cgrt_host_shade_rays")


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_RAYS = np.zeros((16, 7), np.float32)
_RGB = np.zeros((16, 3), np.float32)
_UNITS = np.asarray([[0, 0, 1]], np.float32)
_SPH = np.asarray([[0, 1, 0, 0.1, 1, 1, 1]], np.float32)


def _soft(pkg, **kw):
    f = dict(spherical=_SPH.ctypes.data, unit_vectors=_UNITS.ctypes.data, nspherical=1, samples=4, nunits=1, seed=0, closest_hit=0)
    f.update(kw)
    return C.byref(pkg.SoftShadows(f["spherical"], f["unit_vectors"], f["nspherical"], f["samples"], f["nunits"], f["seed"], f["closest_hit"]))


def _call(pkg, scene, device, rays="ok", n=16, lights="ok", nl=None, soft=None, max_level=2, rgb="ok", handle="ok"):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    args = [
        scene._h if handle == "ok" else None,
        C.c_void_p(_RAYS.ctypes.data) if rays == "ok" else None,
        n,
        None if lights is None else L.ctypes.data_as(C.c_void_p),
        len(L) if nl is None else nl,
        soft,
        max_level,
        C.c_void_p(_RGB.ctypes.data) if rgb == "ok" else None,
    ]
    st = pkg.RenderStats()
    if device:
        return pkg.lib().cgrt_shade_rays_device(*args, None, C.byref(st))
    return pkg.lib().cgrt_shade_rays(*args, C.byref(st))


@pytest.mark.parametrize("device", [False, True])
def test_argument_checks_and_their_order(pkg, host_scene, device):
    assert len(host_scene.sd.point_lights) >= 1
    c = lambda **kw: _call(pkg, host_scene, device, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(soft=_soft(pkg)) == E_NO_DEVICE
    assert c(n=0) == E_NO_DEVICE and c(max_level=0) == E_NO_DEVICE
    # rule 1: NULL scene, rgb, rays with n > 0, lights with nlights > 0
    assert c(handle=None) == E_ARG
    assert c(rgb=None) == E_ARG
    assert c(rays=None) == E_ARG
    assert c(rays=None, n=0) == E_NO_DEVICE, "NULL rays with n == 0 is allowed"
    assert c(lights=None) == E_ARG
    assert c(lights=None, nl=0) == E_NO_DEVICE
    # rule 2: n > 0x7fffffff
    assert c(n=0x80000000) == E_ARG and c(n=1 << 40) == E_ARG
    # rule 3: max_level outside 0..16
    assert c(max_level=-1) == E_ARG and c(max_level=17) == E_ARG
    assert c(max_level=16) == E_NO_DEVICE
    # rule 4: bad soft shadows (cgrt_render_soft's rules)
    for bad in (dict(spherical=None), dict(unit_vectors=None), dict(nunits=0), dict(samples=0), dict(samples=(1 << 24) + 1)):
        assert c(soft=_soft(pkg, **bad)) == E_ARG, bad
    assert c(soft=_soft(pkg, nspherical=0, spherical=None, unit_vectors=None)) == E_NO_DEVICE, "no spherical lights: the table is unused"
    # the order: each rule wins over every later one
    bad_soft = _soft(pkg, samples=0)
    assert c(rgb=None, n=1 << 40, max_level=99, soft=bad_soft) == E_ARG
    assert "NULL" in pkg.lib().cgrt_last_error().decode()
    assert c(n=1 << 40, max_level=99, soft=bad_soft) == E_ARG
    assert "0x7fffffff" in pkg.lib().cgrt_last_error().decode()
    assert c(max_level=99, soft=bad_soft) == E_ARG
    assert "depth" in pkg.lib().cgrt_last_error().decode()
    assert c(soft=bad_soft) == E_ARG
    assert "soft" in pkg.lib().cgrt_last_error().decode()


def test_python_entry_checks(pkg, host_scene):
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.shade_rays(np.zeros((4, 7), np.float32))
    assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        host_scene.shade_rays(np.zeros((4, 6), np.float32))


def test_shade_rays_tensor_rejects_bad_tensors(pkg, host_scene, scene_data):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="host-only"):
        host_scene.shade_rays_tensor(torch.zeros((4, 7)))
    # (a device-backed scene object that never reaches the library: every check below fires first)
    sc = pkg.Scene.__new__(pkg.Scene)
    sc.device = 0
    for bad in (np.zeros((4, 7), np.float32), torch.zeros((4, 6)), torch.zeros((4, 7), dtype=torch.float64), torch.zeros((4, 7)),
                torch.zeros((7, 4)).t()):
        with pytest.raises(ValueError):
            sc.shade_rays_tensor(bad)

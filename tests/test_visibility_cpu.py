"""No GPU: the visibility queries (cgrt_occluded*, cgrt_in_shadow*, cgrt_soft_lit*, include/cgrt.h).

* The six entries and the mirror's C symbols are exported.
* Every argument is checked before any device work, in the documented order, on a host-only scene: each rule is CGRT_E_ARG and
  wins over the ones after it; an otherwise valid call is CGRT_E_NO_DEVICE.
* The *_tensor methods validate their tensors before any call."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_occluded", "cgrt_occluded_device", "cgrt_in_shadow", "cgrt_in_shadow_device", "cgrt_soft_lit", "cgrt_soft_lit_device")


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    H = C.CDLL(pkg.HOST_LIB_PATH)
    for sym in ("cgrt_host_occluded", "cgrt_host_in_shadow", "cgrt_host_soft_lit"):
        assert hasattr(H, sym), sym
    for name in ("occluded", "occluded_device", "occluded_tensor", "in_shadow", "in_shadow_device", "in_shadow_tensor", "soft_lit",
                 "soft_lit_device", "soft_lit_tensor"):
        assert callable(getattr(pkg.Scene, name, None)), name


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_RAYS = np.zeros((16, 7), np.float32)
_PTS = np.zeros((16, 3), np.float32)
_OUT = np.zeros(16 * 8, np.uint32)  # bytes or counts
_UNITS = np.asarray([[0, 0, 1]], np.float32)
_SPH = np.asarray([[0, 1, 0, 0.1, 1, 1, 1], [0, 2, 0, 0.1, 1, 1, 1]], np.float32)
_LIGHTS = np.asarray([[0, 1, 0, 1, 1, 1], [1, 1, 0, 1, 1, 1], [0, 1, 1, 1, 1, 1]], np.float32)
_VP = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731


def _soft(pkg, **kw):
    f = dict(spherical=_SPH.ctypes.data, unit_vectors=_UNITS.ctypes.data, nspherical=2, samples=4, nunits=1, seed=0, closest_hit=0)
    f.update(kw)
    return C.byref(pkg.SoftShadows(f["spherical"], f["unit_vectors"], f["nspherical"], f["samples"], f["nunits"], f["seed"], f["closest_hit"]))


def _occluded(pkg, sc, device, handle="ok", rays="ok", n=16, hit="ok", rays_at=0):
    args = [sc._h if handle == "ok" else None, C.c_void_p(_RAYS.ctypes.data + rays_at) if rays == "ok" else None, n,
            _VP(_OUT) if hit == "ok" else None]
    return pkg.lib().cgrt_occluded_device(*args, None) if device else pkg.lib().cgrt_occluded(*args)


def _in_shadow(pkg, sc, device, handle="ok", points="ok", n=16, lights="ok", nl=3, out="ok", points_at=0):
    args = [sc._h if handle == "ok" else None, C.c_void_p(_PTS.ctypes.data + points_at) if points == "ok" else None, n,
            _VP(_LIGHTS) if lights == "ok" else None, nl, _VP(_OUT) if out == "ok" else None]
    return pkg.lib().cgrt_in_shadow_device(*args, None) if device else pkg.lib().cgrt_in_shadow(*args)


def _soft_lit(pkg, sc, device, handle="ok", points="ok", n=16, soft="ok", lit="ok", points_at=0, lit_at=0):
    args = [sc._h if handle == "ok" else None, C.c_void_p(_PTS.ctypes.data + points_at) if points == "ok" else None, n,
            _soft(pkg) if soft == "ok" else soft, C.c_void_p(_OUT.ctypes.data + lit_at) if lit == "ok" else None]
    return pkg.lib().cgrt_soft_lit_device(*args, None) if device else pkg.lib().cgrt_soft_lit(*args)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


@pytest.mark.parametrize("device", [False, True])
def test_occluded_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _occluded(pkg, host_scene, device, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(n=0) == E_NO_DEVICE and c(n=0x7fffffff) == E_NO_DEVICE
    # rule 1: NULL scene, rays or hit with n > 0
    assert c(handle=None) == E_ARG
    assert c(rays=None) == E_ARG and c(hit=None) == E_ARG
    assert c(rays=None, hit=None, n=0) == E_NO_DEVICE, "NULL arrays with n == 0 are allowed"
    # rule 2: n > 0x7fffffff
    assert c(n=0x80000000) == E_ARG and c(n=1 << 40) == E_ARG
    assert "0x7fffffff" in _err(pkg)
    # rule 3 (device form): d_rays 4-byte aligned
    assert c(rays_at=2) == (E_ARG if device else E_NO_DEVICE)
    # the order
    assert c(handle=None, n=1 << 40, rays_at=2) == E_ARG and "NULL" in _err(pkg)
    assert c(hit=None, n=1 << 40, rays_at=2) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 40, rays_at=2) == E_ARG and "0x7fffffff" in _err(pkg)
    if device:
        assert c(rays_at=2) == E_ARG and "aligned" in _err(pkg)


@pytest.mark.parametrize("device", [False, True])
def test_in_shadow_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _in_shadow(pkg, host_scene, device, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE
    assert c(n=0) == E_NO_DEVICE and c(nl=0) == E_NO_DEVICE
    # rule 1: NULL scene, points or out with n > 0, lights with nlights > 0
    assert c(handle=None) == E_ARG
    assert c(points=None) == E_ARG and c(out=None) == E_ARG
    assert c(lights=None) == E_ARG
    assert c(lights=None, nl=0) == E_NO_DEVICE
    assert c(points=None, out=None, n=0) == E_NO_DEVICE
    # rule 2: n or n * nlights above 0x7fffffff (the bound itself is allowed)
    assert c(n=0x80000000) == E_ARG and c(n=0x80000000, nl=0) == E_ARG
    assert c(n=0x7fffffff, nl=1) == E_NO_DEVICE and c(n=0x7fffffff, nl=2) == E_ARG
    assert c(n=0x7fffffff // 3, nl=3) == E_NO_DEVICE and c(n=0x7fffffff // 3 + 1, nl=3) == E_ARG
    assert "0x7fffffff" in _err(pkg)
    # rule 3 (device form): d_points 4-byte aligned
    assert c(points_at=2) == (E_ARG if device else E_NO_DEVICE)
    # the order
    assert c(lights=None, n=1 << 40, points_at=2) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 40, points_at=2) == E_ARG and "0x7fffffff" in _err(pkg)


@pytest.mark.parametrize("device", [False, True])
def test_soft_lit_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _soft_lit(pkg, host_scene, device, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE
    assert c(n=0) == E_NO_DEVICE and c(soft=None) == E_NO_DEVICE
    assert c(soft=_soft(pkg, nspherical=0, spherical=None, unit_vectors=None)) == E_NO_DEVICE, "no spherical lights: the table is unused"
    # rule 1: NULL scene, points or lit with n > 0
    assert c(handle=None) == E_ARG
    assert c(points=None) == E_ARG and c(lit=None) == E_ARG
    assert c(points=None, lit=None, n=0) == E_NO_DEVICE
    # rule 2: n or n * nspherical above 0x7fffffff
    assert c(n=0x80000000) == E_ARG
    assert c(n=0x7fffffff // 2) == E_NO_DEVICE and c(n=0x7fffffff // 2 + 1) == E_ARG
    # rule 3: bad soft (cgrt_shade_rays' rules)
    for bad in (dict(spherical=None), dict(unit_vectors=None), dict(nunits=0), dict(samples=0), dict(samples=(1 << 24) + 1)):
        assert c(soft=_soft(pkg, **bad)) == E_ARG, bad
    assert c(soft=_soft(pkg, samples=1 << 24)) == E_NO_DEVICE
    # rule 4 (device form): d_points and d_lit 4-byte aligned
    assert c(points_at=2) == (E_ARG if device else E_NO_DEVICE)
    assert c(lit_at=2) == (E_ARG if device else E_NO_DEVICE)
    # the order
    bad_soft = _soft(pkg, samples=0)
    assert c(lit=None, n=1 << 40, soft=bad_soft, points_at=2) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 40, soft=bad_soft, points_at=2) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(soft=bad_soft, points_at=2) == E_ARG and "soft" in _err(pkg)


def test_python_entries_reach_the_library(pkg, host_scene):
    for call in (lambda: host_scene.occluded(np.zeros((4, 7), np.float32)), lambda: host_scene.in_shadow(np.zeros((4, 3), np.float32)),
                 lambda: host_scene.soft_lit(np.zeros((4, 3), np.float32), _SPH, _UNITS, samples=4)):
        with pytest.raises(pkg.CgrtError) as e:
            call()
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        host_scene.occluded(np.zeros((4, 6), np.float32))


def test_tensor_methods_reject_bad_tensors(pkg, host_scene):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="host-only"):
        host_scene.occluded_tensor(torch.zeros((4, 7)))
    with pytest.raises(ValueError, match="host-only"):
        host_scene.in_shadow_tensor(torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="host-only"):
        host_scene.soft_lit_tensor(torch.zeros((4, 3)), _SPH, _UNITS)
    # (a device-backed scene object that never reaches the library: every check below fires first)
    sc = pkg.Scene.__new__(pkg.Scene)
    sc.device = 0
    sc.sd = host_scene.sd
    calls = {
        "occluded": (7, lambda x, **kw: sc.occluded_tensor(x, **kw)),
        "in_shadow": (3, lambda x, **kw: sc.in_shadow_tensor(x, lights=_LIGHTS, **kw)),
        "soft_lit": (3, lambda x, **kw: sc.soft_lit_tensor(x, _SPH, _UNITS, samples=4, **kw)),
    }
    for name, (w, f) in calls.items():
        for bad in (np.zeros((4, w), np.float32), torch.zeros((4, w + 1)), torch.zeros((4, w), dtype=torch.float64), torch.zeros((4, w)),
                    torch.zeros((w, 4)).t()):
            with pytest.raises(ValueError):
                f(bad)


"""No GPU: light sets (include/cgrt.h cgrt_render_light_sets, cgrt_render_light_sets_device).

* Both entries are exported and bound.
* Each checks its arguments before any device work on a host-only scene: every malformed argument is CGRT_E_ARG (NULL scene / cam /
  sets / output, nsets 0 or above 1024, offsets that do not start at 0 or that decrease, NULL lights or spherical with a count, spherical
  lights without a valid soft or with a soft that carries lights of its own, W or H <= 0, max_level, W*H too large, a bad format, lists the
  32-bit indices cannot address), an otherwise valid call CGRT_E_NO_DEVICE.
* Scene.render_light_sets* raise ValueError before any native call for sequences of different lengths, bad shapes and a wrong `out`."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_render_light_sets", "cgrt_render_light_sets_device")


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


class _Sets:
    """CSR arrays of B sets (set b: b % 3 point lights, and with sph=True one spherical light in every other set), kept alive."""

    def __init__(self, B=3, sph=False, nlights=None):
        n = [b % 3 for b in range(B)] if nlights is None else nlights
        self.lights = np.arange(max(sum(n), 1) * 6, dtype=np.float32).reshape(-1, 6)
        self.loff = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
        ns = [b % 2 for b in range(B)] if sph else [0] * B
        self.sph = np.ones((max(sum(ns), 1), 7), np.float32)
        self.soff = np.concatenate([[0], np.cumsum(ns)]).astype(np.uint32)
        self.B = B
        self.has_sph = sph

    def struct(self, pkg, nsets=None, lights="ok", loff="ok", sph="ok", soff="ok"):
        p = lambda a, k: None if k is None else (a.ctypes.data if isinstance(k, str) else k.ctypes.data)  # noqa: E731
        return pkg.LightSets(self.B if nsets is None else nsets, p(self.lights, lights), p(self.loff, loff),
                             p(self.sph, sph) if self.has_sph else None, p(self.soff, soff) if self.has_sph else None)


def _soft(pkg, **over):
    units = pkg.unit_vector_table(64, 0)
    q = dict(spherical=None, unit_vectors=units.ctypes.data, nspherical=0, samples=4, nunits=len(units), seed=0, closest_hit=0)
    q.update(over)
    return pkg.SoftShadows(**q), units


def _call(pkg, scene, entry, sets, W=8, H=8, cam="ok", soft=None, max_level=2, out="ok", fmt=0, handle="ok", q=None):
    c = pkg.Camera.from_array(pkg.scenes.default_camera(W if W > 0 else 8, H if H > 0 else 8))
    cp = C.byref(c) if cam == "ok" else None
    qq = sets.struct(pkg) if q is None else q
    sp = C.byref(qq) if q != "null" else None
    d_out = None if out is None else C.c_void_p(_OUT.ctypes.data + (0 if out == "ok" else out))
    h = scene._h if handle == "ok" else None
    st = pkg.RenderStats()
    sq = None if soft is None else C.byref(soft)
    lib = pkg.lib()
    if entry == "host":
        return lib.cgrt_render_light_sets(h, cp, W, H, sp, sq, max_level, d_out, C.byref(st))
    return lib.cgrt_render_light_sets_device(h, cp, W, H, sp, sq, max_level, d_out, fmt, None, C.byref(st))


@pytest.mark.parametrize("entry", ["host", "device"])
def test_argument_checks(pkg, host_scene, entry):
    err = pkg.lib().cgrt_last_error
    S = _Sets()
    call = lambda **kw: _call(pkg, host_scene, entry, kw.pop("sets", S), **kw)  # noqa: E731
    assert call() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert b"host-only" in err()
    assert call(sets=_Sets(1)) == E_NO_DEVICE  # one set without lights
    assert call(sets=_Sets(1024)) == E_NO_DEVICE
    soft, keep = _soft(pkg)
    assert call(sets=_Sets(4, sph=True), soft=soft) == E_NO_DEVICE
    assert call(soft=soft) == E_NO_DEVICE, "soft may accompany sets without spherical lights"
    # NULL scene, camera, sets, output
    assert call(handle=None) == E_ARG
    assert call(cam=None) == E_ARG
    assert call(q="null") == E_ARG
    assert call(out=None) == E_ARG
    # nsets
    assert call(q=S.struct(pkg, nsets=0)) == E_ARG
    assert b"nsets" in err()
    big = _Sets(1025)
    assert call(sets=big, q=big.struct(pkg)) == E_ARG
    assert b"nsets" in err()
    # offsets
    assert call(q=S.struct(pkg, loff=None)) == E_ARG
    assert call(q=S.struct(pkg, loff=np.array([1, 1, 2, 4], np.uint32))) == E_ARG
    assert b"start at 0" in err()
    assert call(q=S.struct(pkg, loff=np.array([0, 2, 1, 3], np.uint32))) == E_ARG
    assert b"decrease" in err()
    T = _Sets(4, sph=True)
    assert call(sets=T, soft=soft, q=T.struct(pkg, soff=np.array([2, 2, 2, 2, 2], np.uint32))) == E_ARG
    assert call(sets=T, soft=soft, q=T.struct(pkg, soff=np.array([0, 1, 0, 1, 2], np.uint32))) == E_ARG
    # NULL light arrays with a count (and none needed without one)
    assert call(q=S.struct(pkg, lights=None)) == E_ARG
    assert b"lights is NULL" in err()
    Z = _Sets(3, nlights=[0, 0, 0])
    assert call(sets=Z, q=Z.struct(pkg, lights=None)) == E_NO_DEVICE
    assert call(sets=T, soft=soft, q=T.struct(pkg, sph=None)) == E_ARG
    # spherical lights need a valid soft without lights of its own
    assert call(sets=T, soft=None) == E_ARG
    for bad in (dict(unit_vectors=None), dict(nunits=0), dict(samples=0), dict(samples=(1 << 24) + 1)):
        b, _k = _soft(pkg, **bad)
        assert call(sets=T, soft=b) == E_ARG, bad
    sph = np.ones((1, 7), np.float32)
    own, _k = _soft(pkg, spherical=sph.ctypes.data, nspherical=1)
    assert call(sets=T, soft=own) == E_ARG
    assert call(soft=own) == E_ARG
    own0, _k = _soft(pkg, spherical=sph.ctypes.data, nspherical=0)
    assert call(soft=own0) == E_ARG
    # frame and depth
    assert call(W=0) == E_ARG
    assert call(H=-1) == E_ARG
    assert call(max_level=-1) == E_ARG
    assert call(max_level=17) == E_ARG
    assert call(max_level=16) == E_NO_DEVICE
    assert call(W=65536, H=32768) == E_ARG  # W*H > 0x7fffffff
    # lists the 32-bit indices cannot address: W*H x distinct positions
    many = _Sets(1, nlights=[64])
    assert call(sets=many, W=8192, H=8192) == E_ARG
    assert b"32-bit" in err()
    same = _Sets(1, nlights=[64])
    same.lights[:] = same.lights[0]  # 64 lights at ONE position: one shadow ray per hit
    assert call(sets=same, W=8192, H=8192) == E_NO_DEVICE
    if entry == "device":
        assert call(fmt=3) == E_ARG
        assert call(fmt=-1) == E_ARG
        assert call(out=2) == E_ARG  # not 4-byte aligned
        for fmt in (0, 1, 2):
            assert call(fmt=fmt) == E_NO_DEVICE


def test_python_value_errors_before_any_call(pkg, host_scene, monkeypatch):
    sc = host_scene
    cam = pkg.scenes.default_camera(8, 8)
    called = []
    real = pkg.lib()

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real, name)

    monkeypatch.setattr(pkg, "lib", lambda: Spy())
    L = np.zeros((1, 6), np.float32)
    with pytest.raises(ValueError):
        sc.render_light_sets(cam, 8, 8, [L, L], spherical_sets=[np.zeros((1, 7), np.float32)], units=np.ones((4, 3), np.float32))
    with pytest.raises(ValueError):
        sc.render_light_sets(cam, 8, 8, [np.zeros((2, 5), np.float32)])
    with pytest.raises(ValueError):
        sc.render_light_sets(cam, 8, 8, [np.zeros(6, np.float32)])
    with pytest.raises(ValueError):
        sc.render_light_sets(cam, 8, 8, [L], spherical_sets=[np.zeros((1, 6), np.float32)])
    with pytest.raises(ValueError):
        sc.render_light_sets_device(cam, 8, 8, 0, [L, L], spherical_sets=[])
    with pytest.raises(ValueError):
        sc.render_light_sets_tensor(cam, 8, 8, [L, L], spherical_sets=[None])
    with pytest.raises(ValueError):
        sc.render_light_sets_tensor(cam, 8, 8, [np.zeros((1, 7), np.float32)])
    with pytest.raises(ValueError):
        sc.render_light_sets_tensor(cam, 8, 8, [L], format="bgr")
    assert called == [], f"native calls before the ValueError: {called}"


def test_python_out_checks(pkg, host_scene):
    torch = pytest.importorskip("torch")
    sc = host_scene
    cam = pkg.scenes.default_camera(8, 4)
    L = np.zeros((1, 6), np.float32)
    sets = [L, L, L]
    for out, fmt in (
        (torch.zeros((2, 4, 8, 3)), "rgb"),  # batch count
        (torch.zeros((3, 4, 8, 4)), "rgb"),  # shape
        (torch.zeros((3, 4, 8, 3), dtype=torch.float64), "rgb"),  # dtype
        (torch.zeros((3, 4, 8, 4), dtype=torch.float32), "rgba8"),
        (torch.zeros((3, 8, 4, 3)).transpose(1, 2), "rgb"),  # not contiguous
        (torch.zeros((3, 3, 4, 8)), "chw"),  # a CPU tensor
        (np.zeros((3, 4, 8, 3), np.float32), "rgb"),
    ):
        with pytest.raises(ValueError):
            sc.render_light_sets_tensor(cam, 8, 4, sets, format=fmt, out=out)

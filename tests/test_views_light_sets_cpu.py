"""No GPU: multi-view light sets (include/cgrt.h cgrt_render_views_light_sets, cgrt_render_views_light_sets_device,
cgrt_enqueue_render_views_light_sets_device).

* The three entries are exported and bound.
* Each checks its arguments before any device work on a host-only scene, in the header's order: every malformed argument is CGRT_E_ARG
  (NULL scene / cams / sets / output, nviews 0, the sets' rules, W or H <= 0, max_level, nviews*W*H and the super-tiles, the lists' 32-bit
  bounds and the samples bound over all views, nviews*nsets*W*H, a bad format or alignment), each limit is tested on both sides, a call
  with two faults reports the earlier one, and an otherwise valid call is CGRT_E_NO_DEVICE.
* The Scene methods raise ValueError before any native call for bad cameras, bad sets and a wrong (V, S, ...) `out`."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_render_views_light_sets", "cgrt_render_views_light_sets_device", "cgrt_enqueue_render_views_light_sets_device")
METHODS = ("render_views_light_sets", "render_views_light_sets_device", "render_views_light_sets_tensor", "enqueue_render_views_light_sets_tensor")


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym)
    for m in METHODS:
        assert callable(getattr(pkg.Scene, m))


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_OUT = np.zeros(64, np.float32)  # a non-NULL output: every call here fails before anything is written


class _Sets:
    """CSR arrays of B sets (set b: b % 3 point lights at distinct positions, or `nlights`; with sph=True one spherical light in every other
    set), kept alive."""

    def __init__(self, B=3, sph=False, nlights=None, nsph=None):
        n = [b % 3 for b in range(B)] if nlights is None else nlights
        self.lights = np.arange(max(sum(n), 1) * 6, dtype=np.float32).reshape(-1, 6)
        self.loff = np.concatenate([[0], np.cumsum(n)]).astype(np.uint32)
        ns = ([b % 2 for b in range(B)] if nsph is None else nsph) if sph else [0] * B
        self.sph = np.arange(max(sum(ns), 1) * 7, dtype=np.float32).reshape(-1, 7)
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


_CAMS = {}


def _cams(pkg, V):
    if V not in _CAMS:
        c = np.asarray(pkg.scenes.default_camera(8, 8), np.float32)
        _CAMS[V] = np.ascontiguousarray(np.tile(c.reshape(1, 9), (max(V, 1), 1)))
    return _CAMS[V]


def _call(pkg, scene, entry, sets, V=2, W=8, H=8, cams="ok", soft=None, max_level=2, out="ok", fmt=0, handle="ok", q=None):
    cp = _cams(pkg, V).ctypes.data if cams == "ok" else None
    qq = sets.struct(pkg) if q is None else q
    sp = C.byref(qq) if q != "null" else None
    d_out = None if out is None else C.c_void_p(_OUT.ctypes.data + (0 if out == "ok" else out))
    h = scene._h if handle == "ok" else None
    sq = None if soft is None else C.byref(soft)
    lib = pkg.lib()
    if entry == "host":
        return lib.cgrt_render_views_light_sets(h, cp, V, W, H, sp, sq, max_level, d_out, C.byref(pkg.RenderStats()))
    if entry == "device":
        return lib.cgrt_render_views_light_sets_device(h, cp, V, W, H, sp, sq, max_level, d_out, fmt, None, C.byref(pkg.RenderStats()))
    t = C.c_uint64(0)
    rc = lib.cgrt_enqueue_render_views_light_sets_device(h, cp, V, W, H, sp, sq, max_level, d_out, fmt, None, C.byref(t))
    assert rc == 0 or t.value == 0, "a refused batch issues no ticket"
    return rc


@pytest.mark.parametrize("entry", ["host", "device", "enqueue"])
def test_argument_checks(pkg, host_scene, entry):
    err = pkg.lib().cgrt_last_error
    S = _Sets()
    call = lambda **kw: _call(pkg, host_scene, entry, kw.pop("sets", S), **kw)  # noqa: E731
    assert call() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert b"host-only" in err()
    assert call(V=1) == E_NO_DEVICE
    assert call(sets=_Sets(1)) == E_NO_DEVICE  # one set without lights
    assert call(sets=_Sets(1024)) == E_NO_DEVICE
    soft, keep = _soft(pkg)
    assert call(sets=_Sets(4, sph=True), soft=soft) == E_NO_DEVICE
    assert call(soft=soft) == E_NO_DEVICE, "soft may accompany sets without spherical lights"
    # NULL scene, cameras, sets, output
    assert call(handle=None) == E_ARG
    assert call(cams=None) == E_ARG
    assert call(q="null") == E_ARG
    assert call(out=None) == E_ARG
    assert b"NULL" in err()
    # nviews
    assert call(V=0) == E_ARG
    assert b"nviews" in err()
    # the sets' rules
    assert call(q=S.struct(pkg, nsets=0)) == E_ARG
    assert b"nsets" in err()
    big = _Sets(1025)
    assert call(sets=big, q=big.struct(pkg)) == E_ARG
    assert b"nsets" in err()
    assert call(q=S.struct(pkg, loff=None)) == E_ARG
    assert call(q=S.struct(pkg, loff=np.array([1, 1, 2, 4], np.uint32))) == E_ARG
    assert b"start at 0" in err()
    assert call(q=S.struct(pkg, loff=np.array([0, 2, 1, 3], np.uint32))) == E_ARG
    assert b"decrease" in err()
    T = _Sets(4, sph=True)
    assert call(sets=T, soft=soft, q=T.struct(pkg, soff=np.array([0, 1, 0, 1, 2], np.uint32))) == E_ARG
    assert call(q=S.struct(pkg, lights=None)) == E_ARG
    assert b"lights is NULL" in err()
    Z = _Sets(3, nlights=[0, 0, 0])
    assert call(sets=Z, q=Z.struct(pkg, lights=None)) == E_NO_DEVICE
    assert call(sets=T, soft=soft, q=T.struct(pkg, sph=None)) == E_ARG
    assert call(sets=T, soft=None) == E_ARG
    for bad in (dict(unit_vectors=None), dict(nunits=0), dict(samples=0), dict(samples=(1 << 24) + 1)):
        b, _k = _soft(pkg, **bad)
        assert call(sets=T, soft=b) == E_ARG, bad
    sph = np.ones((1, 7), np.float32)
    own, _k = _soft(pkg, spherical=sph.ctypes.data, nspherical=1)
    assert call(soft=own) == E_ARG
    # frame and depth
    assert call(W=0) == E_ARG
    assert call(H=-1) == E_ARG
    assert b"frame size" in err()
    assert call(max_level=-1) == E_ARG
    assert call(max_level=17) == E_ARG
    assert b"depth" in err()
    assert call(max_level=16) == E_NO_DEVICE
    assert call(max_level=0) == E_NO_DEVICE
    # nviews * W * H, both sides of the limit
    assert call(V=2, W=32768, H=32768) == E_ARG
    assert b"nviews*W*H" in err()
    assert call(V=1, W=32768, H=32768, sets=_Sets(1, nlights=[0])) == E_NO_DEVICE  # 2^30 pixels, 2^18 super-tiles
    # super-tiles over all views: a 65 x 65 view is 2 x 2 super-tiles
    assert call(V=65537, W=65, H=65) == E_ARG
    assert b"super-tiles" in err()
    assert call(V=65536, W=65, H=65) == E_NO_DEVICE
    # the shadow list over ALL views: V*W*H x distinct positions
    many = _Sets(1, nlights=[32])
    assert call(sets=many, V=4, W=4096, H=4096) == E_ARG
    assert b"32-bit" in err()
    assert call(sets=many, V=2, W=4096, H=4096) == E_NO_DEVICE  # (2^25 x 32 = 2^30)
    same = _Sets(1, nlights=[32])
    same.lights[:] = same.lights[0]  # 32 lights at ONE position: one shadow ray per hit
    assert call(sets=same, V=4, W=4096, H=4096) == E_NO_DEVICE
    # the soft-shadow counters over all views: V*W*H x distinct keys
    keys = _Sets(1, sph=True, nsph=[32])
    assert call(sets=keys, soft=soft, V=4, W=4096, H=4096) == E_ARG
    assert b"32-bit" in err()
    assert call(sets=keys, soft=soft, V=2, W=4096, H=4096) == E_NO_DEVICE
    # and the samples bound (V*W*H x keys x samples above 64 x 0x7fffffff)
    one = _Sets(1, sph=True, nsph=[1])
    many_smp, _k = _soft(pkg, samples=1 << 24)
    assert call(sets=one, soft=many_smp, V=8, W=1024, H=1024) == E_ARG
    assert b"32-bit" in err()
    assert call(sets=one, soft=many_smp, V=1, W=64, H=64) == E_NO_DEVICE
    # nviews * nsets * W * H
    assert call(sets=_Sets(3, nlights=[0, 0, 0]), V=1, W=30000, H=30000) == E_ARG
    assert b"nviews*nsets*W*H" in err()
    assert call(sets=_Sets(2, nlights=[0, 0]), V=1, W=30000, H=30000) == E_NO_DEVICE
    if entry != "host":
        assert call(fmt=3) == E_ARG
        assert call(fmt=-1) == E_ARG
        assert b"format" in err()
        assert call(out=2) == E_ARG  # not 4-byte aligned
        assert b"aligned" in err()
        for fmt in (0, 1, 2):
            assert call(fmt=fmt) == E_NO_DEVICE
    # the order: with two faults, the earlier check answers
    assert call(cams=None, V=0) == E_ARG and b"NULL" in err()
    assert call(V=0, q=S.struct(pkg, nsets=0)) == E_ARG and b"nviews" in err()
    assert call(q=S.struct(pkg, nsets=0), W=0) == E_ARG and b"nsets" in err()
    assert call(W=0, max_level=17) == E_ARG and b"frame size" in err()
    assert call(max_level=17, V=2, W=32768, H=32768) == E_ARG and b"depth" in err()
    assert call(sets=many, V=2, W=32768, H=32768) == E_ARG and b"nviews*W*H" in err()
    assert call(sets=_Sets(3, nlights=[32, 0, 0]), V=1, W=30000, H=30000) == E_ARG and b"32-bit" in err()
    if entry != "host":
        assert call(sets=_Sets(3, nlights=[0, 0, 0]), V=1, W=30000, H=30000, fmt=3) == E_ARG and b"nviews*nsets*W*H" in err()
        assert call(fmt=3, handle="ok") == E_ARG, "CGRT_E_ARG before CGRT_E_NO_DEVICE"


def test_python_value_errors_before_any_call(pkg, host_scene, monkeypatch):
    sc = host_scene
    cam = pkg.scenes.default_camera(8, 8)
    cams = [cam, cam]
    called = []
    real = pkg.lib()

    class Spy:
        def __getattr__(self, name):
            called.append(name)
            return getattr(real, name)

    monkeypatch.setattr(pkg, "lib", lambda: Spy())
    L = np.zeros((1, 6), np.float32)
    sph = [np.zeros((1, 7), np.float32)]
    for m in ("render_views_light_sets", "render_views_light_sets_tensor", "enqueue_render_views_light_sets_tensor"):
        f = getattr(sc, m)
        with pytest.raises(ValueError):
            f(cams, 8, 8, [L, L], spherical_sets=sph, units=np.ones((4, 3), np.float32))  # sets of different lengths
        with pytest.raises(ValueError):
            f(cams, 8, 8, [np.zeros((2, 5), np.float32)])
        with pytest.raises(ValueError):
            f(cams, 8, 8, [L], spherical_sets=[np.zeros((1, 6), np.float32)])
        with pytest.raises(ValueError):
            f(np.zeros((2, 8), np.float32), 8, 8, [L])  # cameras of the wrong width
        with pytest.raises(ValueError):
            f(np.zeros(9, np.float32), 8, 8, [L])
    with pytest.raises(ValueError):
        sc.render_views_light_sets_device(cams, 8, 8, 0, [L, L], spherical_sets=[])
    for m in ("render_views_light_sets_tensor", "enqueue_render_views_light_sets_tensor"):
        with pytest.raises(ValueError):
            getattr(sc, m)(cams, 8, 8, [L], format="bgr")
    assert called == [], f"native calls before the ValueError: {called}"


@pytest.mark.parametrize("method", ["render_views_light_sets_tensor", "enqueue_render_views_light_sets_tensor"])
def test_python_out_checks(pkg, host_scene, method):
    torch = pytest.importorskip("torch")
    f = getattr(host_scene, method)
    cam = pkg.scenes.default_camera(8, 4)
    cams = [cam, cam]
    L = np.zeros((1, 6), np.float32)
    sets = [L, L, L]  # V = 2, S = 3
    for out, fmt in (
        (torch.zeros((3, 2, 4, 8, 3)), "rgb"),  # (S, V) instead of (V, S)
        (torch.zeros((6, 4, 8, 3)), "rgb"),  # a flat batch
        (torch.zeros((2, 2, 4, 8, 3)), "rgb"),  # set count
        (torch.zeros((2, 3, 4, 8, 4)), "rgb"),  # shape
        (torch.zeros((2, 3, 4, 8, 3), dtype=torch.float64), "rgb"),  # dtype
        (torch.zeros((2, 3, 4, 8, 4), dtype=torch.float32), "rgba8"),
        (torch.zeros((2, 3, 3, 8, 4)), "chw"),  # (H, W) swapped
        (torch.zeros((2, 3, 8, 4, 3)).transpose(2, 3), "rgb"),  # not contiguous
        (torch.zeros((2, 3, 3, 4, 8)), "chw"),  # a CPU tensor
        (torch.zeros((2, 3, 4, 8, 4), dtype=torch.uint8), "rgba8"),  # a CPU tensor
        (np.zeros((2, 3, 4, 8, 3), np.float32), "rgb"),
    ):
        with pytest.raises(ValueError):
            f(cams, 8, 4, sets, format=fmt, out=out)

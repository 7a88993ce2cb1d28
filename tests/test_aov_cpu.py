"""No GPU: geometry buffers of a device frame (include/cgrt.h CgrtAovOut, cgrt_*_aov_device).

* The four entries are exported and bound.
* On a host-only scene each entry checks its counterpart's arguments first, in the counterpart's order, then its own -- aov NULL, no plane
  requested, max_level 0, aa with nranks > 1, a misaligned plane -- all CGRT_E_ARG; an otherwise valid call is CGRT_E_NO_DEVICE.
* The tensor wrappers refuse a wrong `aovs` / `aov_out` with ValueError before any call."""
import ctypes as C

import numpy as np
import pytest

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_render_aov_device", "cgrt_render_views_aov_device", "cgrt_enqueue_render_aov_device", "cgrt_enqueue_render_views_aov_device")
PLANES = ("depth", "normal", "position", "albedo", "prim_id", "material_id", "mask")


def test_new_symbols_are_exported_and_bound(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
        assert getattr(pkg.lib(), sym).argtypes[-1] is not None and len(getattr(pkg.lib(), sym).argtypes) >= 14
    assert pkg.AOV_NAMES == PLANES
    assert C.sizeof(pkg.AovOut) == 7 * C.sizeof(C.c_void_p) + 8  # seven pointers, an int, padding
    for name in ("render_aov_device", "render_views_aov_device", "render_aov_tensor", "render_views_aov_tensor", "enqueue_render_aov_tensor",
                 "enqueue_render_views_aov_tensor"):
        assert callable(getattr(pkg.Scene, name))


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_BUF = np.zeros(256, np.float32)  # non-NULL addresses: every call here fails before anything is written


def _aov(pkg, planes=("depth",), offset=0, chw=0):
    return pkg.AovOut.from_pointers({k: _BUF.ctypes.data + 16 + offset for k in planes}, bool(chw))


def _call(pkg, scene, entry, W=8, H=8, lights="ok", nl=None, max_level=2, aa=0, rank=0, nranks=1, out="ok", fmt=0, row_bytes=0, cam="ok",
          handle="ok", aov="ok", nviews=2):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    lights_p = None if lights is None else L.ctypes.data_as(C.c_void_p)
    nl = len(L) if nl is None else nl
    d_out = None if out is None else C.c_void_p(_BUF.ctypes.data + (0 if out == "ok" else out))
    a = _aov(pkg) if aov == "ok" else aov
    a = None if a is None else C.byref(a)
    h = scene._h if handle == "ok" else None
    st, t = pkg.RenderStats(), C.c_uint64()
    tail = C.byref(t) if "enqueue" in entry else C.byref(st)
    f = getattr(pkg.lib(), entry)
    if "views" in entry:
        cams = pkg.camera_array([pkg.scenes.default_camera(max(W, 1), max(H, 1))] * max(nviews, 1))
        return f(h, cams.ctypes.data_as(C.c_void_p) if cam == "ok" else None, nviews, W, H, lights_p, nl, None, max_level, d_out, fmt, None, tail, a)
    c = pkg.Camera.from_array(pkg.scenes.default_camera(max(W, 1), max(H, 1)))
    return f(h, C.byref(c) if cam == "ok" else None, W, H, lights_p, nl, None, max_level, aa, rank, nranks, d_out, fmt, row_bytes, None, tail, a)


@pytest.mark.parametrize("entry", ENTRIES)
def test_counterpart_checks_come_first(pkg, host_scene, entry):
    """Each of the counterpart's bad arguments is CGRT_E_ARG with the counterpart's message even when the planes are bad too."""
    bad_aov = None
    err = pkg.lib().cgrt_last_error
    assert _call(pkg, host_scene, entry) == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert b"host-only" in err()
    assert _call(pkg, host_scene, entry, handle=None, aov=bad_aov) == E_ARG
    assert _call(pkg, host_scene, entry, cam=None, aov=bad_aov) == E_ARG and b"aov" not in err()
    assert _call(pkg, host_scene, entry, out=None, aov=bad_aov) == E_ARG and b"aov" not in err()
    assert _call(pkg, host_scene, entry, lights=None, aov=bad_aov) == E_ARG and b"lights" in err()
    assert _call(pkg, host_scene, entry, W=0, aov=bad_aov) == E_ARG and b"aov" not in err()
    for ml in (-1, 17):
        assert _call(pkg, host_scene, entry, max_level=ml, aov=bad_aov) == E_ARG and b"depth" in err()
    for fmt in (3, -1):
        assert _call(pkg, host_scene, entry, fmt=fmt, aov=bad_aov) == E_ARG and b"format" in err()
    assert _call(pkg, host_scene, entry, out=2, aov=bad_aov) == E_ARG and b"aligned" in err() and b"geometry" not in err()
    if "views" in entry:
        assert _call(pkg, host_scene, entry, nviews=0, aov=bad_aov) == E_ARG and b"aov" not in err()
    else:
        for rank, nranks in ((1, 1), (-1, 2), (2, 2), (0, 0)):
            assert _call(pkg, host_scene, entry, rank=rank, nranks=nranks, aov=bad_aov) == E_ARG and b"rank" in err()
        assert _call(pkg, host_scene, entry, row_bytes=12 * 8 - 4, aov=bad_aov) == E_ARG and b"row_bytes" in err()
        assert _call(pkg, host_scene, entry, aa=1, W=23171, H=23171, aov=bad_aov) == E_ARG and b"0x7fffffff" in err()


@pytest.mark.parametrize("entry", ENTRIES)
def test_plane_checks(pkg, host_scene, entry):
    err = pkg.lib().cgrt_last_error
    assert _call(pkg, host_scene, entry, aov=None) == E_ARG and b"aov is NULL" in err()
    assert _call(pkg, host_scene, entry, aov=pkg.AovOut()) == E_ARG and b"no plane" in err()
    assert _call(pkg, host_scene, entry, aov=pkg.AovOut(chw=1)) == E_ARG and b"no plane" in err()
    assert _call(pkg, host_scene, entry, max_level=0) == E_ARG and b"max_level 0" in err()
    assert _call(pkg, host_scene, entry, max_level=1) == E_NO_DEVICE
    assert _call(pkg, host_scene, entry, max_level=16) == E_NO_DEVICE
    for k in PLANES:  # each plane alone, both layouts
        for chw in (0, 1):
            assert _call(pkg, host_scene, entry, aov=_aov(pkg, (k,), chw=chw)) == E_NO_DEVICE, k
    assert _call(pkg, host_scene, entry, aov=_aov(pkg, PLANES)) == E_NO_DEVICE
    for k in PLANES[:-1]:  # 4-byte elements
        for off in (1, 2, 3):
            assert _call(pkg, host_scene, entry, aov=_aov(pkg, (k,), offset=off)) == E_ARG and b"aligned to its element size" in err(), (k, off)
    for off in (1, 2, 3):  # the mask is bytes
        assert _call(pkg, host_scene, entry, aov=_aov(pkg, ("mask",), offset=off)) == E_NO_DEVICE
    # the documented order among the planes' own checks: NULL, no plane, depth 0, aa with ranks, alignment
    assert _call(pkg, host_scene, entry, max_level=0, aov=pkg.AovOut()) == E_ARG and b"no plane" in err()
    assert _call(pkg, host_scene, entry, max_level=0, aov=_aov(pkg, ("depth",), offset=2)) == E_ARG and b"max_level 0" in err()
    if "views" not in entry:
        assert _call(pkg, host_scene, entry, aa=1) == E_NO_DEVICE
        assert _call(pkg, host_scene, entry, rank=1, nranks=2) == E_NO_DEVICE
        assert _call(pkg, host_scene, entry, aa=1, rank=1, nranks=2) == E_ARG and b"nranks == 1" in err()
        assert _call(pkg, host_scene, entry, aa=1, rank=0, nranks=3, max_level=0) == E_ARG and b"max_level 0" in err()
        assert _call(pkg, host_scene, entry, aa=1, rank=0, nranks=3, aov=_aov(pkg, ("normal",), offset=1)) == E_ARG and b"nranks == 1" in err()


def test_aov_pointer_dict(pkg):
    a = pkg.AovOut.from_pointers({"depth": 64, "mask": 7, "normal": 0, "albedo": None}, chw=True)
    assert (a.depth, a.mask, a.normal, a.albedo, a.position, a.chw) == (64, 7, None, None, None, 1)
    with pytest.raises(ValueError, match="unknown"):
        pkg.AovOut.from_pointers({"colour": 64})


def test_tensor_wrappers_reject_bad_planes(pkg, host_scene):
    torch = pytest.importorskip("torch")
    W, H = 8, 6
    cam = pkg.scenes.default_camera(W, H)
    cams = [cam, cam, cam]
    single = (lambda **kw: host_scene.render_aov_tensor(cam, W, H, **kw), lambda **kw: host_scene.enqueue_render_aov_tensor(cam, W, H, **kw))
    views = (lambda **kw: host_scene.render_views_aov_tensor(cams, W, H, **kw), lambda **kw: host_scene.enqueue_render_views_aov_tensor(cams, W, H, **kw))
    for lead, calls in (((), single), ((3,), views)):
        for f in calls:
            with pytest.raises(ValueError, match="subset"):
                f(aovs=("depth", "colour"))
            with pytest.raises(ValueError, match="subset"):
                f(aovs=())
            with pytest.raises(ValueError, match="subset"):
                f(aovs=("depth", "depth"))
            with pytest.raises(ValueError, match="requested"):
                f(aovs=("depth",), aov_out={"mask": torch.zeros(lead + (H, W), dtype=torch.uint8)})
            with pytest.raises(ValueError, match="torch tensor"):
                f(aovs=("depth",), aov_out={"depth": np.zeros(lead + (H, W), np.float32)})
            with pytest.raises(ValueError, match="dtype"):
                f(aovs=("depth",), aov_out={"depth": torch.zeros(lead + (H, W), dtype=torch.float64)})
            with pytest.raises(ValueError, match="dtype"):
                f(aovs=("prim_id",), aov_out={"prim_id": torch.zeros(lead + (H, W), dtype=torch.int64)})
            with pytest.raises(ValueError, match="dtype"):
                f(aovs=("mask",), aov_out={"mask": torch.zeros(lead + (H, W), dtype=torch.bool)})
            with pytest.raises(ValueError, match="shape"):
                f(aovs=("depth",), aov_out={"depth": torch.zeros(lead + (W, H), dtype=torch.float32)})
            with pytest.raises(ValueError, match="shape"):  # (H, W, 3) where chw asks for (3, H, W), and the other way round
                f(aovs=("normal",), chw=True, aov_out={"normal": torch.zeros(lead + (H, W, 3), dtype=torch.float32)})
            with pytest.raises(ValueError, match="shape"):
                f(aovs=("albedo",), aov_out={"albedo": torch.zeros(lead + (3, H, W), dtype=torch.float32)})
            with pytest.raises(ValueError, match="contiguous"):
                f(aovs=("position",), aov_out={"position": torch.zeros(lead + (H, W, 6), dtype=torch.float32)[..., ::2]})
            with pytest.raises(ValueError, match="cuda"):  # right in every other respect, but a CPU tensor
                f(aovs=("material_id",), aov_out={"material_id": torch.zeros(lead + (H, W), dtype=torch.int32)})
    # aa: the planes are the sub-sample frame's
    for f in single:
        with pytest.raises(ValueError, match="shape"):
            f(aovs=("depth",), aa=True, aov_out={"depth": torch.zeros((H, W), dtype=torch.float32)})
        with pytest.raises(ValueError, match="cuda"):
            f(aovs=("depth",), aa=True, aov_out={"depth": torch.zeros((2 * H, 2 * W), dtype=torch.float32)})

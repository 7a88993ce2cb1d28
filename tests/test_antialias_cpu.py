"""No GPU: the anti-aliased frame entries (cgrt_render_aa*, the reference's antiAliasing branch, src/main.cpp:663-687).

* Finding AA3 of include/cgrt.h bit for bit: the reference's sub-pixel ndc of sub-sample (xc, yc) of a W x H frame,
  float(xc) / W * (2.0f / level) - 1.0f with level = 2.0f, equals the ndc the library's camera computes for pixel (xc, yc) of a
  2W x 2H frame, float(xc) / float(2W) * 2.0f - 1.0f (walk_exact.h primary_ray), for every xc.
* The new C-ABI entries check every argument before any device work, on a host-only scene."""
import ctypes as C

import numpy as np
import pytest

F32 = np.float32
SIZES = [1, 2, 3, 61, 97, 256, 800, 1080, 1920, 2160, 3840, 4095]


def _upstream_ndc(c, n):
    """main.cpp:670-672: float(xc) / W * (2.0f / level) - 1.0f, level = 2.0f (W an int converted to float by the division)."""
    level = F32(2.0)
    return (c.astype(F32) / F32(n)) * (F32(2.0) / level) - F32(1.0)


def _library_ndc(c, n2):
    """walk_exact.h primary_ray for pixel c of a frame n2 = 2n wide: float(x) / float(W) * 2.0f - 1.0f."""
    return (c.astype(F32) / F32(n2)) * F32(2.0) - F32(1.0)


def _check_size(n):
    c = np.arange(2 * n, dtype=np.int64)  # xc in {2x, 2x + 1}, x < n
    a, b = _upstream_ndc(c, n), _library_ndc(c, 2 * n)
    assert a.dtype == F32 and b.dtype == F32
    bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
    assert bad.size == 0, f"n={n}: sub-sample {c[bad[0]]} upstream {a[bad[0]]!r} library {b[bad[0]]!r}"


@pytest.mark.parametrize("n", SIZES)
def test_subsample_ndc_equals_double_frame_ndc(n):
    _check_size(n)


def test_subsample_ndc_random_sizes_up_to_8192():
    rng = np.random.default_rng(663)
    for n in sorted(set(rng.integers(1, 8193, 200).tolist()) | {8191, 8192}):
        _check_size(int(n))


def test_resolve_reference_order(pkg):
    """resolve_aa (the numpy statement the GPU tests compare against) sums in the reference's loop order and divides by 5.0f."""
    rng = np.random.default_rng(5)
    W, H = 5, 3
    sub = rng.random((4 * W * H, 3), dtype=np.float32) * F32(3)
    got = pkg.resolve_aa(sub, W, H)
    s = sub.reshape(2 * H, 2 * W, 3)
    for y in range(H):
        for x in range(W):
            acc = np.zeros(3, F32)
            for yc in (2 * y, 2 * y + 1):
                for xc in (2 * x, 2 * x + 1):
                    acc = acc + s[yc, xc]
            want = acc / F32(5.0)
            assert np.array_equal(got[y * W + x].view(np.uint32), want.view(np.uint32))
    # / 5.0f, not * 0.2f: the two differ for some values, and the resolve must be the division
    v = np.arange(1, 4001, dtype=F32) * F32(0.37)
    assert np.any((v / F32(5.0)).view(np.uint32) != (v * F32(0.2)).view(np.uint32))


# ---- argument checks of cgrt_render_aa / cgrt_render_aa_mapped / cgrt_render_multi_aa (host-only scene) ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


def _args(pkg, sd, W=8, H=8, lights="ok"):
    cam = pkg.Camera.from_array(pkg.scenes.default_camera(W, H))
    L = np.ascontiguousarray(sd.point_lights, np.float32).reshape(-1, 6)
    lp = None if lights is None else L.ctypes.data_as(C.c_void_p)
    return cam, L, lp


def _aa(pkg, scene, W=8, H=8, nl=None, lights="ok", rank=0, nranks=1):
    cam, L, lp = _args(pkg, scene.sd, W, H, lights)
    rgb = np.zeros((3, 3), np.float32)  # never written: every call here fails before any work
    st = pkg.RenderStats()
    return pkg.lib().cgrt_render_aa(scene._h, C.byref(cam), W, H, lp, len(L) if nl is None else nl, None, 2, rank, nranks,
                                    rgb.ctypes.data_as(C.c_void_p), C.byref(st))


def _aa_mapped(pkg, scene, W=8, H=8, nl=None, lights="ok"):
    cam, L, lp = _args(pkg, scene.sd, W, H, lights)
    ptr = C.c_void_p()
    return pkg.lib().cgrt_render_aa_mapped(scene._h, C.byref(cam), W, H, lp, len(L) if nl is None else nl, None, 2, C.byref(ptr), None)


def _aa_multi(pkg, scenes, W=8, H=8, nl=None, lights="ok", nscenes=None):
    cam, L, lp = _args(pkg, scenes[0].sd, W, H, lights)
    arr = (C.c_void_p * max(1, len(scenes)))(*[s._h for s in scenes])
    rgb = np.zeros((3, 3), np.float32)
    return pkg.lib().cgrt_render_multi_aa(arr, len(scenes) if nscenes is None else nscenes, C.byref(cam), W, H, lp,
                                          len(L) if nl is None else nl, None, 2, rgb.ctypes.data_as(C.c_void_p), None)


def test_render_aa_rejects_bad_arguments(pkg, host_scene):
    assert len(host_scene.sd.point_lights) >= 1
    assert _aa(pkg, host_scene) == -2, "host-only scene: CGRT_E_NO_DEVICE"
    assert b"host-only" in pkg.lib().cgrt_last_error()
    assert _aa(pkg, host_scene, lights=None) == -1, "lights missing"
    assert _aa(pkg, host_scene, W=0) == -1 and _aa(pkg, host_scene, H=-3) == -1
    assert _aa(pkg, host_scene, W=23171, H=23171) == -1, "4*W*H overflows the frame limit"
    assert b"0x7fffffff" in pkg.lib().cgrt_last_error()
    assert _aa(pkg, host_scene, W=1 << 15, H=1 << 14) == -1  # 4*W*H = 2^31
    assert _aa(pkg, host_scene, W=(1 << 15) - 1, H=1 << 14) == -2  # 4*W*H < 2^31: only the missing device remains
    for rank, nranks in ((1, 1), (-1, 2), (2, 2), (0, 0)):
        assert _aa(pkg, host_scene, rank=rank, nranks=nranks) == -1, (rank, nranks)
    assert _aa(pkg, host_scene, rank=1, nranks=2) == -2
    cam = pkg.Camera.from_array(pkg.scenes.default_camera(8, 8))
    assert pkg.lib().cgrt_render_aa(None, C.byref(cam), 8, 8, None, 0, None, 2, 0, 1, None, None) == -1
    assert pkg.lib().cgrt_render_aa(host_scene._h, None, 8, 8, None, 0, None, 2, 0, 1, None, None) == -1


def test_render_aa_mapped_rejects_bad_arguments(pkg, host_scene):
    assert _aa_mapped(pkg, host_scene) == -2
    assert _aa_mapped(pkg, host_scene, lights=None) == -1
    assert _aa_mapped(pkg, host_scene, W=0) == -1
    assert _aa_mapped(pkg, host_scene, W=40000, H=20000) == -1
    cam = pkg.Camera.from_array(pkg.scenes.default_camera(8, 8))
    assert pkg.lib().cgrt_render_aa_mapped(host_scene._h, C.byref(cam), 8, 8, None, 0, None, 2, None, None) == -1


def test_render_multi_aa_rejects_bad_arguments(pkg, scene_data, host_scene):
    other = pkg.Scene(scene_data("cube"), device=-1)
    try:
        two = [host_scene, other]
        assert _aa_multi(pkg, two) == -2
        assert _aa_multi(pkg, two, lights=None) == -1
        assert _aa_multi(pkg, two, W=-1) == -1
        assert _aa_multi(pkg, two, W=23171, H=23171) == -1
        assert _aa_multi(pkg, two, nscenes=0) == -1, "no replica"
        assert _aa_multi(pkg, two, nscenes=65) == -1, "more replicas than ranks allowed"
        assert _aa_multi(pkg, [host_scene, host_scene]) == -1, "the same replica twice"
    finally:
        other.close()


def test_python_render_aa_on_host_only_scene_raises(pkg, host_scene):
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.render_aa(pkg.scenes.default_camera(8, 8), 8, 8)
    assert e.value.args and "host-only" in str(e.value)
    with pytest.raises(pkg.CgrtError):
        pkg.render_multi_aa([host_scene], pkg.scenes.default_camera(8, 8), 8, 8)

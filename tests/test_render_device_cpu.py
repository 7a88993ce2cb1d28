"""No GPU: shaded frames into device memory (cgrt_render_device, include/cgrt.h CGRT_FRAME_*).

* Both new symbols are exported (cgrt_render_device, cgrt_debug_export_frame).
* cgrt_render_device checks every argument before any device work, in cgrt_render_aa's order, on a host-only scene: each bad argument
  is CGRT_E_ARG, an otherwise valid call CGRT_E_NO_DEVICE.
* The numpy statement of CGRT_FRAME_RGBA8 the GPU tests compare against (rgba8_of) equals the C++ mirror's own BMP writer
  (Screen::writeBitmapToFile, screen.cpp:38-49) byte for byte on a frame of edge values: every k/255 boundary and its float32
  neighbours, +-0, denormals, 1 - ulp, 1, 1 + ulp, large values and +-inf (not NaN: upstream's cast of NaN is undefined).
* Scene.render_tensor validates a caller's tensor before any call."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

F32 = np.float32
E_ARG, E_NO_DEVICE = -1, -2


def test_new_symbols_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ("cgrt_render_device", "cgrt_debug_export_frame"):
        assert sym in pkg.EXPORTS and hasattr(L, sym)
    assert pkg.FRAME_FORMATS == {"rgb": 0, "chw": 1, "rgba8": 2}


# ---- argument checks (host-only scene) ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_OUT = np.zeros(64, np.float32)  # a non-NULL d_out: every call here fails before anything is written


def _dev(pkg, scene, W=8, H=8, lights="ok", nl=None, soft=None, max_level=2, aa=0, rank=0, nranks=1, out="ok", fmt=0, row_bytes=0,
         cam="ok", handle="ok"):
    L = np.ascontiguousarray(scene.sd.point_lights, np.float32).reshape(-1, 6)
    c = pkg.Camera.from_array(pkg.scenes.default_camera(max(W, 1), max(H, 1)))
    if out == "ok":
        d_out = C.c_void_p(_OUT.ctypes.data)
    elif out is None:
        d_out = None
    else:
        d_out = C.c_void_p(_OUT.ctypes.data + out)  # (a byte offset)
    st = pkg.RenderStats()
    return pkg.lib().cgrt_render_device(
        scene._h if handle == "ok" else None, C.byref(c) if cam == "ok" else None, W, H,
        None if lights is None else L.ctypes.data_as(C.c_void_p), len(L) if nl is None else nl, soft, max_level, aa, rank, nranks,
        d_out, fmt, row_bytes, None, C.byref(st),
    )  # fmt: skip


def test_render_device_argument_order(pkg, host_scene):
    assert len(host_scene.sd.point_lights) >= 1
    for aa in (0, 1):
        assert _dev(pkg, host_scene, aa=aa) == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
        assert b"host-only" in pkg.lib().cgrt_last_error()
        for fmt in (0, 1, 2):
            assert _dev(pkg, host_scene, aa=aa, fmt=fmt) == E_NO_DEVICE
        assert _dev(pkg, host_scene, aa=aa, handle=None) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, cam=None) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, out=None) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, lights=None) == E_ARG, "lights missing"
        assert _dev(pkg, host_scene, aa=aa, lights=None, nl=0) == E_NO_DEVICE, "no lights at all is a valid frame"
        assert _dev(pkg, host_scene, aa=aa, W=0) == E_ARG and _dev(pkg, host_scene, aa=aa, H=-3) == E_ARG
        for ml in (-1, 17):
            assert _dev(pkg, host_scene, aa=aa, max_level=ml) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, max_level=16) == E_NO_DEVICE
        for rank, nranks in ((1, 1), (-1, 2), (2, 2), (0, 0)):
            assert _dev(pkg, host_scene, aa=aa, rank=rank, nranks=nranks) == E_ARG, (rank, nranks)
        assert _dev(pkg, host_scene, aa=aa, rank=1, nranks=2) == E_NO_DEVICE
        for fmt in (3, -1, 7):
            assert _dev(pkg, host_scene, aa=aa, fmt=fmt) == E_ARG, fmt
            assert b"format" in pkg.lib().cgrt_last_error()
        W = 8
        for fmt, row in ((0, 12 * W), (1, 4 * W), (2, 4 * W)):
            assert _dev(pkg, host_scene, aa=aa, fmt=fmt, row_bytes=row - 4) == E_ARG, "row_bytes below the packed row"
            assert _dev(pkg, host_scene, aa=aa, fmt=fmt, row_bytes=row + 2) == E_ARG, "row_bytes not a multiple of 4"
            assert _dev(pkg, host_scene, aa=aa, fmt=fmt, row_bytes=row) == E_NO_DEVICE
            assert _dev(pkg, host_scene, aa=aa, fmt=fmt, row_bytes=row + 20) == E_NO_DEVICE
        assert _dev(pkg, host_scene, aa=aa, out=2) == E_ARG, "d_out not 4-byte aligned"
    # the AA frame limit (4*W*H sub-samples) applies with aa only
    assert _dev(pkg, host_scene, aa=1, W=23171, H=23171) == E_ARG
    assert b"0x7fffffff" in pkg.lib().cgrt_last_error()
    assert _dev(pkg, host_scene, aa=1, W=(1 << 15) - 1, H=1 << 14) == E_NO_DEVICE
    assert _dev(pkg, host_scene, aa=0, W=23171, H=23171) == E_NO_DEVICE


def test_render_device_rejects_bad_soft_shadows(pkg, host_scene):
    sph = np.zeros((1, 7), np.float32)
    units = np.zeros((4, 3), np.float32)

    def soft(spherical=True, units_=True, samples=16, nunits=4):
        return C.byref(pkg.SoftShadows(sph.ctypes.data if spherical else None, units.ctypes.data if units_ else None, 1, samples, nunits, 0, 0))

    for aa in (0, 1):
        assert _dev(pkg, host_scene, aa=aa, soft=soft()) == E_NO_DEVICE
        assert _dev(pkg, host_scene, aa=aa, soft=soft(spherical=False)) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, soft=soft(units_=False)) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, soft=soft(nunits=0)) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, soft=soft(samples=0)) == E_ARG
        assert _dev(pkg, host_scene, aa=aa, soft=soft(samples=(1 << 24) + 1)) == E_ARG


def test_debug_export_rejects_bad_arguments(pkg):
    rgb = np.zeros((6, 3), np.float32)
    out = np.zeros(256, np.uint8)
    f = pkg.lib().cgrt_debug_export_frame
    assert f(0, rgb.ctypes.data_as(C.c_void_p), 3, 2, 3, 0, out.ctypes.data_as(C.c_void_p)) == E_ARG
    assert f(0, rgb.ctypes.data_as(C.c_void_p), 3, 2, 0, 35, out.ctypes.data_as(C.c_void_p)) == E_ARG
    assert f(0, rgb.ctypes.data_as(C.c_void_p), 3, 2, 2, 14, out.ctypes.data_as(C.c_void_p)) == E_ARG
    assert f(0, None, 3, 2, 0, 0, out.ctypes.data_as(C.c_void_p)) == E_ARG
    assert f(0, rgb.ctypes.data_as(C.c_void_p), 3, 0, 0, 0, out.ctypes.data_as(C.c_void_p)) == E_ARG


# ---- the RGBA8 statement against the C++ mirror's BMP writer ----
def edge_values() -> np.ndarray:
    """float32 values that pin the clamp-and-truncate conversion: every k/255 and its 3 neighbours on each side, the values v around
    each k where float32(v * 255) reaches k, +-0, denormals, 1 - ulp, 1, 1 + ulp, large values, +-inf (no NaN)."""
    vals = []
    for k in range(256):
        for v in (F32(k) / F32(255), F32(k / 255.0)):
            x = v
            for _ in range(4):
                vals.append(x)
                x = np.nextafter(x, F32(-np.inf), dtype=F32)
            x = v
            for _ in range(4):
                vals.append(x)
                x = np.nextafter(x, F32(np.inf), dtype=F32)
        if k:  # the first float32 whose product with 255 rounds to at least k
            lo, hi = F32(0), F32(2)
            while np.nextafter(lo, hi, dtype=F32) < hi:
                mid = F32((float(lo) + float(hi)) / 2)
                if mid <= lo or mid >= hi:
                    break
                if F32(mid * F32(255)) >= F32(k):
                    hi = mid
                else:
                    lo = mid
            vals += [lo, hi]
    tiny = np.finfo(F32).tiny
    one = F32(1)
    vals += [F32(0), F32(-0.0), F32(1.4e-45), F32(-1.4e-45), np.nextafter(tiny, F32(0), dtype=F32), tiny, -tiny,
             np.nextafter(one, F32(0), dtype=F32), one, np.nextafter(one, F32(2), dtype=F32), F32(1.5), F32(255), F32(1e30),
             np.finfo(F32).max, -np.finfo(F32).max, F32(np.inf), F32(-np.inf), F32(-0.5), F32(-1e-7)]
    a = np.asarray(vals, np.float32)
    assert not np.isnan(a).any()
    return a


def edge_frame(W=37):
    """The edge values laid out as a W x H float frame (odd W), the rest zero; returns (rgb[W*H, 3], W, H)."""
    v = edge_values()
    H = -(-len(v) // (3 * W))
    rgb = np.zeros(W * H * 3, np.float32)
    rgb[: len(v)] = v
    return rgb.reshape(-1, 3), W, H


def read_bmp24(path):
    """(H, W, 3) bytes of a 24-bit bottom-up BMP in storage order (row r of the file = frame row r), BGR."""
    data = open(path, "rb").read()
    off, W, H, bpp = struct.unpack_from("<I", data, 10)[0], *struct.unpack_from("<ii", data, 18), struct.unpack_from("<H", data, 28)[0]
    assert bpp == 24 and H > 0
    row = (3 * W + 3) & ~3
    rows = np.frombuffer(data, np.uint8, count=row * H, offset=off).reshape(H, row)
    return rows[:, : 3 * W].reshape(H, W, 3)


def test_rgba8_statement_equals_the_mirrors_bmp_writer(pkg, tmp_path):
    rgb, W, H = edge_frame()
    path = str(tmp_path / "edge.bmp")
    pkg.host_write_bmp(path, rgb, W, H)
    bgr = read_bmp24(path)
    got = pkg.rgba8_of(rgb, W, H)
    assert got.shape == (H, W, 4) and got.dtype == np.uint8
    assert (got[..., 3] == 255).all()
    # RGBA8 row H-1-y is frame row y; BMP storage row r is frame row r, bytes B, G, R
    want = bgr[::-1, :, ::-1]
    bad = np.argwhere(got[..., :3] != want)
    assert bad.size == 0, f"first difference at {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    # the statement spans every byte value and truncates (0.5 / 255 -> 0, 254.99 / 255 -> 254)
    assert set(np.unique(got[..., :3]).tolist()) == set(range(256))
    one = pkg.rgba8_of(np.array([[0.5 / 255, 254.99 / 255, 2.0]], np.float32), 1, 1)
    assert one.tolist() == [[[0, 254, 255, 255]]]


def test_rgba8_statement_maps_nan_to_zero(pkg):
    rgb = np.array([[np.nan, -np.nan, 0.5], [np.inf, -np.inf, 1.0]], np.float32)
    got = pkg.rgba8_of(rgb, 2, 1)
    assert got.tolist() == [[[0, 0, 127, 255], [255, 0, 255, 255]]]


# ---- render_tensor validates its `out` before any call ----
def test_render_tensor_rejects_bad_out(pkg, host_scene):
    torch = pytest.importorskip("torch")
    cam = pkg.scenes.default_camera(8, 6)
    W, H = 8, 6
    for fmt, shape, dtype in (("rgb", (H, W, 3), torch.float32), ("chw", (3, H, W), torch.float32), ("rgba8", (H, W, 4), torch.uint8)):
        with pytest.raises(ValueError, match="cuda"):  # right dtype and shape, but a CPU tensor
            host_scene.render_tensor(cam, W, H, format=fmt, out=torch.zeros(shape, dtype=dtype))
        with pytest.raises(ValueError, match="dtype"):
            host_scene.render_tensor(cam, W, H, format=fmt, out=torch.zeros(shape, dtype=torch.float64))
        with pytest.raises(ValueError, match="shape"):
            host_scene.render_tensor(cam, W, H, format=fmt, out=torch.zeros((H + 1,) + tuple(shape[1:]), dtype=dtype))
        with pytest.raises(ValueError, match="shape"):
            host_scene.render_tensor(cam, W, H, format=fmt, out=torch.zeros(shape[::-1], dtype=dtype))
    with pytest.raises(ValueError, match="format"):
        host_scene.render_tensor(cam, W, H, format="bgr")
    with pytest.raises(ValueError):
        host_scene.render_tensor(cam, W, H, out=np.zeros((H, W, 3), np.float32))


def test_package_import_stays_torch_free():
    """Importing the package does not import torch (render_tensor imports it when called)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys, __graft_entry__ as e; e.load_package(); print('torch' in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "False"


def test_single_runtime_check_reads_maps_until_it_succeeds(pkg, monkeypatch):
    """render_tensor's check of the process's HIP runtimes parses /proc/self/maps, which costs about as much as a frame's host
    overhead: it runs until it first succeeds, not on every frame, and a failure is not remembered."""
    calls = []
    answers = [["/a/libamdhip64.so", "/b/libamdhip64.so"], ["/a/libamdhip64.so"]]
    monkeypatch.setattr(pkg, "_one_runtime_seen", False)
    monkeypatch.setattr(pkg, "hip_runtimes", lambda: calls.append(1) or answers[min(len(calls), 2) - 1])
    with pytest.raises(RuntimeError, match="2 HIP runtimes"):
        pkg._check_one_hip_runtime()
    for _ in range(5):
        pkg._check_one_hip_runtime()
    assert len(calls) == 2

"""GPU tests of shaded frames written straight into device memory (cgrt_render_device / Scene.render_device / Scene.render_tensor).

The float formats must hold the bit patterns of the host entries' frame (cgrt_render / cgrt_render_soft / cgrt_render_aa), the 8-bit
format the numpy statement rgba8_of (which tests/test_render_device_cpu.py ties to the C++ mirror's BMP writer) of that frame, byte for
byte.  Every output is checked with sentinel-filled memory around it: the export writes the frame's (owned) pixels and nothing else."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from test_render_device_cpu import edge_frame, read_bmp24

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PREDICTED = 1
FORMATS = ("rgb", "chw", "rgba8")


def _cam(pkg, name, W, H):
    if name == "spheres":  # (as tests/test_antialias_gpu.py)
        return np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
    return pkg.scenes.default_camera(W, H)


def _moved(pkg, W, H, i):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[3] += np.float32(0.03 * i)  # (euler x)
    cam[4] += np.float32(0.05 * i)
    return cam


def _soft(pkg):
    return dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(4096, 3), samples=16, seed=11)


def _reference(sc, cam, W, H, aa, depth=2, lights=None, soft=None):
    """The host entries' frame: (rgb[W*H, 3], stats)."""
    soft = soft or {}
    if aa:
        return sc.render_aa(cam, W, H, max_level=depth, lights=lights, **soft)
    if soft:
        return sc.render_soft(cam, W, H, max_level=depth, lights=lights, **soft)
    return sc.render(cam, W, H, max_level=depth, lights=lights)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _as_rgb(a, fmt, W, H):
    """A float output in the (W*H, 3) layout of the host entries."""
    return np.ascontiguousarray(a.transpose(1, 2, 0) if fmt == "chw" else a).reshape(W * H, 3)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _owned(W, H, aa, rank, nranks):
    """(H, W) mask of the pixels `rank` owns: 64x64 super-tiles, or (aa) 32x32-pixel blocks, row-major, index % nranks == rank."""
    T = 32 if aa else 64
    y, x = np.mgrid[0:H, 0:W]
    return ((y // T) * (-(-W // T)) + x // T) % nranks == rank


GRID = [("cube", 64, 48, 2), ("monkey", 80, 64, 2), ("spheres", 72, 40, 2), ("cornell", 96, 64, 2), ("cornell", 96, 64, 4),
        ("cornell", 97, 61, 2), ("monkey", 1, 1, 2), ("cornell", 3, 1, 4), ("cornell", 800, 800, 2)]  # fmt: skip


@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("name,W,H,depth", GRID)
def test_float_formats_bit_identical(pkg, scene_data, name, W, H, depth, aa):
    sc = pkg.Scene(scene_data(name), device=0)
    cam = _cam(pkg, name, W, H)
    softs = [None] + ([_soft(pkg)] if name == "cornell" and W * H <= 97 * 61 else [])
    for soft in softs:
        want, st_want = _reference(sc, cam, W, H, aa, depth, soft=soft)
        for fmt in ("rgb", "chw"):
            t, st = sc.render_tensor(cam, W, H, format=fmt, aa=aa, max_level=depth, **(soft or {}))
            assert t.shape == ((3, H, W) if fmt == "chw" else (H, W, 3)) and t.dtype == torch.float32 and t.device.index == 0
            assert _same_bits(_as_rgb(_host(t), fmt, W, H), want), (fmt, soft is not None)
            for k in ("primary_rays", "shadow_rays", "reflection_rays", "levels", "soft_shadow_rays"):
                assert st[k] == st_want[k], k


def test_rgba8_equals_statement(pkg, scene_data):
    clamped = False
    for name, W, H, aa in (("spheres", 72, 40, False), ("cornell", 97, 61, False), ("cornell", 97, 61, True), ("monkey", 80, 64, True)):
        sd = scene_data(name)
        sc = pkg.Scene(sd, device=0)
        cam = _cam(pkg, name, W, H)
        for colour in (None, 15.0):
            lights = None
            if colour is not None:  # bright lights: channels above 1 exercise the clamp
                lights = np.asarray(sd.point_lights, np.float32).reshape(-1, 6).copy()
                lights[:, 3:6] = colour
            want, _ = _reference(sc, cam, W, H, aa, lights=lights)
            clamped = clamped or bool((want > 1).any())
            t, _ = sc.render_tensor(cam, W, H, format="rgba8", aa=aa, lights=lights)
            assert t.shape == (H, W, 4) and t.dtype == torch.uint8
            assert np.array_equal(_host(t), pkg.rgba8_of(want, W, H)), (name, aa, colour)
    assert clamped


def test_rgba8_equals_the_mirrors_bmp(pkg, scene_data, tmp_path):
    """Cornell 480 x 270: the RGB bytes of the device's RGBA8 frame are the BMP the C++ mirror writes (Screen::writeBitmapToFile)."""
    sd = scene_data("cornell")
    W, H = 480, 270
    cam = pkg.scenes.default_camera(W, H)
    path = str(tmp_path / "cornell.bmp")
    pkg.host_render_bmp(sd, cam, W, H, path)
    bgr = read_bmp24(path)  # row r = frame row r
    sc = pkg.Scene(sd, device=0)
    t, _ = sc.render_tensor(cam, W, H, format="rgba8")
    got = _host(t)
    assert np.array_equal(got[::-1, :, :3], bgr[:, :, ::-1])
    assert (got[..., 3] == 255).all() and got[..., :3].any()


def _edge_frame_with_nans():
    rgb, W, H = edge_frame(37)
    flat = rgb.reshape(-1).copy()
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FA00000, 0xFFFFFFFF, 0x7F800001], np.uint32).view(np.float32)  # quiet, negative, signalling
    flat[-len(nans) - 7 : -7] = nans
    return flat.reshape(-1, 3), W, H


@pytest.mark.parametrize("W,pad", [(37, 20), (36, 16), (36, 4)])
def test_debug_export_edge_values(pkg, W, pad):
    """Every format of the export kernel on the edge-value frame (+ NaNs -> 0 in RGBA8), odd and even W, padded rows (16-B aligned
    and not): the written bytes are the statement's, the padding keeps its sentinel."""
    rgb37, _, _ = _edge_frame_with_nans()
    vals = rgb37.reshape(-1)
    H = -(-len(vals) // (3 * W))
    rgb = np.zeros(W * H * 3, np.float32)
    rgb[: len(vals)] = vals
    rgb = rgb.reshape(-1, 3)
    assert np.isnan(rgb).any()
    for fmt in FORMATS:
        row = W * (12 if fmt == "rgb" else 4)
        pitch = row + pad
        rows = 3 * H if fmt == "chw" else H
        n = pitch * (rows - 1) + row
        out = np.full(n, 0xAB, np.uint8)
        pkg.debug_export_frame(rgb, W, H, format=fmt, row_bytes=pitch, out=out)
        full = np.concatenate([out, np.full(pitch * rows - n, 0xAB, np.uint8)]).reshape(rows, pitch)
        assert (full[:, row:] == 0xAB).all(), fmt
        body = full[:, :row]
        if fmt == "rgba8":
            assert np.array_equal(body.reshape(H, W, 4), pkg.rgba8_of(rgb, W, H))
            nan_px = np.isnan(rgb.reshape(H, W, 3))[::-1]
            assert (body.reshape(H, W, 4)[..., :3][nan_px] == 0).all() and nan_px.any()
        else:
            f = np.ascontiguousarray(body).view(np.float32).reshape(rows, -1)
            got = f.reshape(H, W, 3) if fmt == "rgb" else f.reshape(3, H, W).transpose(1, 2, 0)
            assert np.array_equal(got.reshape(-1, 3).view(np.uint32), rgb.view(np.uint32)), fmt


@pytest.mark.parametrize("aa", [False, True])
def test_pitch_leaves_padding_untouched(pkg, scene_data, aa):
    sc = pkg.Scene(scene_data("cornell"), device=0)
    W, H = 97, 61
    cam = pkg.scenes.default_camera(W, H)
    want, _ = _reference(sc, cam, W, H, aa)
    sentinel = {torch.float32: -7.25, torch.uint8: 0xAB}
    for fmt in FORMATS:
        if fmt == "chw":  # rows padded, planes H rows apart
            canvas = torch.full((3, H, W + 11), sentinel[torch.float32], dtype=torch.float32, device="cuda:0")
            view = canvas[:, :, 5 : 5 + W]
        else:
            c = 4 if fmt == "rgba8" else 3
            dt = torch.uint8 if fmt == "rgba8" else torch.float32
            canvas = torch.full((H + 6, W + 11, c), sentinel[dt], dtype=dt, device="cuda:0")
            view = canvas[3 : 3 + H, 5 : 5 + W]
        t, _ = sc.render_tensor(cam, W, H, format=fmt, out=view, aa=aa)
        assert t.data_ptr() == view.data_ptr()
        whole = _host(canvas)
        mask = np.ones(whole.shape, bool)
        if fmt == "chw":
            mask[:, :, 5 : 5 + W] = False
            got = _as_rgb(whole[:, :, 5 : 5 + W], fmt, W, H)
        else:
            mask[3 : 3 + H, 5 : 5 + W] = False
            got = whole[3 : 3 + H, 5 : 5 + W]
        s = sentinel[torch.uint8 if fmt == "rgba8" else torch.float32]
        assert (whole[mask] == s).all(), fmt
        if fmt == "rgba8":
            assert np.array_equal(got, pkg.rgba8_of(want, W, H))
        else:
            assert _same_bits(got.reshape(-1, 3), want)


def _delay_cycles(ms):
    """torch.cuda._sleep cycles that keep a stream busy for about `ms` milliseconds, from a timed delay of 1 M cycles (the counter's
    rate is the device's, not assumed)."""
    s = torch.cuda.Stream(device=0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        torch.cuda._sleep(1_000_000)
        e1.record()
    e1.synchronize()
    per_ms = 1_000_000 / max(e0.elapsed_time(e1), 1e-3)
    return int(per_ms * ms)


@pytest.mark.parametrize("aa", [False, True])
def test_stream_hazard(pkg, scene_data, aa):
    """A non-blocking stream busy with a bounded delay: frame A's export waits behind it, frame B is rendered right away.  The scene's
    own event keeps B's kernels off the workspace until A's export has read it; a fill queued before the call is overwritten."""
    sc = pkg.Scene(scene_data("cornell"), device=0)
    W, H = 200, 120
    camA, camB = _moved(pkg, W, H, 0), _moved(pkg, W, H, 3)
    wantA, _ = _reference(sc, camA, W, H, aa)
    wantB, _ = _reference(sc, camB, W, H, aa)
    assert not _same_bits(wantA, wantB)
    s = torch.cuda.Stream(device=0)
    # the delay must outlast the host-blocking call that renders frame A by a wide margin: 20 x that call's time, at least 100 ms
    # (capped at 2 s), measured on this device and host
    warm = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc.render_tensor(camA, W, H, out=warm, stream=s, aa=aa)
    call_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    cycles = _delay_cycles(min(2000.0, max(100.0, 20.0 * call_ms)))
    outs = {}
    for fmt in ("rgb", "rgba8"):
        shape, dt = ((H, W, 4), torch.uint8) if fmt == "rgba8" else ((H, W, 3), torch.float32)
        outA = torch.zeros(shape, dtype=dt, device="cuda:0")
        outB = torch.zeros(shape, dtype=dt, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            outA.fill_(3)  # queued before the call: the frame must overwrite it
        sc.render_tensor(camA, W, H, format=fmt, out=outA, stream=s, aa=aa)
        pending = torch.cuda.Event()
        pending.record(s)
        assert not pending.query(), "the delay must still hold frame A's export when frame B is rendered"
        sc.render_tensor(camB, W, H, format=fmt, out=outB, stream=s, aa=aa)
        outs[fmt] = (_host(outA), _host(outB))
    assert _same_bits(outs["rgb"][0].reshape(-1, 3), wantA)
    assert _same_bits(outs["rgb"][1].reshape(-1, 3), wantB)
    assert np.array_equal(outs["rgba8"][0], pkg.rgba8_of(wantA, W, H))
    assert np.array_equal(outs["rgba8"][1], pkg.rgba8_of(wantB, W, H))


@pytest.mark.parametrize("aa", [False, True])
def test_ranks_write_only_their_pixels(pkg, scene_data, aa):
    sc = pkg.Scene(scene_data("cornell"), device=0)
    W, H, n = 200, 150, 3
    cam = pkg.scenes.default_camera(W, H)
    want, _ = _reference(sc, cam, W, H, aa)
    for fmt in ("rgb", "rgba8"):
        dt, c, s = (torch.uint8, 4, 0xAB) if fmt == "rgba8" else (torch.float32, 3, -7.25)
        canvas = torch.full((H, W, c), s, dtype=dt, device="cuda:0")
        before = _host(canvas)
        for rank in range(n):
            sc.render_tensor(cam, W, H, format=fmt, out=canvas, aa=aa, rank=rank, nranks=n)
            after = _host(canvas)
            own = _owned(W, H, aa, rank, n)
            if fmt == "rgba8":
                own = own[::-1]
            changed = (after != before).any(axis=2)
            assert not changed[~own].any(), (fmt, rank)
            assert np.array_equal(after[~own], before[~own])
            before = after
        if fmt == "rgba8":
            assert np.array_equal(before, pkg.rgba8_of(want, W, H))
        else:
            assert _same_bits(before.reshape(-1, 3), want)
    # a fresh tensor of a rank: zeros outside its pixels
    t, st = sc.render_tensor(cam, W, H, aa=aa, rank=1, nranks=n)
    got = _host(t)
    own = _owned(W, H, aa, 1, n)
    assert not got[~own].any() and _same_bits(got[own], want.reshape(H, W, 3)[own])
    assert st["primary_rays"] == own.sum() * (4 if aa else 1)


def test_predicted_frames_and_host_entries_between(pkg, scene_data):
    sd = scene_data("cornell")
    W, H = 160, 96
    ref_scene = pkg.Scene(sd, device=0)
    sc = pkg.Scene(sd, device=0)
    cams = [_moved(pkg, W, H, i) for i in range(4)]
    refs = [ref_scene.render(c, W, H)[0] for c in cams]
    outs, paths = [], []
    for i, cam in enumerate(cams):
        t, _ = sc.render_tensor(cam, W, H)
        paths.append(sc.last_render_path())
        outs.append(t)
        got, _ = sc.render(cam, W, H)
        assert _same_bits(got, refs[i])
        got, _ = sc.render_mapped(cams[(i + 1) % 4], W, H)
        assert _same_bits(got, refs[(i + 1) % 4])
    for i, t in enumerate(outs):
        assert _same_bits(_host(t).reshape(-1, 3), refs[i]), i
    assert 0 not in paths[1:] and PREDICTED in paths, paths  # (frames after the first take the predicted path)


def test_render_tensor_defaults_and_raw_pointers(pkg, scene_data):
    sc = pkg.Scene(scene_data("monkey"), device=0)
    W, H = 96, 72
    cam = pkg.scenes.default_camera(W, H)
    for fmt in FORMATS:
        t1, st1 = sc.render_tensor(cam, W, H, format=fmt)
        out = torch.empty_like(t1)
        t2, st2 = sc.render_tensor(cam, W, H, format=fmt, out=out, stream=torch.cuda.current_stream())
        assert t2 is out and t1.data_ptr() != t2.data_ptr()
        assert np.array_equal(_host(t1).view(np.uint8), _host(t2).view(np.uint8)), fmt
        assert st1["primary_rays"] == st2["primary_rays"] == W * H
    assert len(pkg.hip_runtimes()) == 1
    # raw integers: a buffer from the runtime libcgrt.so uses (hipMalloc), the default stream
    hip = C.CDLL(pkg.LIB_PATH)
    want, _ = sc.render(cam, W, H)
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(W * H * 12)) == 0
    try:
        st = sc.render_device(cam, W, H, buf.value)
        assert st["primary_rays"] == W * H
        got = np.empty((W * H, 3), np.float32)
        assert hip.hipMemcpy(C.c_void_p(got.ctypes.data), buf, C.c_size_t(W * H * 12), 2) == 0  # (device to host, synchronous)
        assert _same_bits(got, want)
    finally:
        assert hip.hipFree(buf) == 0


_EXPANDABLE = r"""
import os, sys
import torch  # (first: torch's HIP runtime is the one libcgrt.so binds to)
sys.path.insert(0, os.environ["CGRT_ROOT"])
import numpy as np
import __graft_entry__ as e
pkg = e.load_package()
sd = pkg.scenes.SceneData.load(os.path.join(os.environ["CGRT_ROOT"], "tests", "golden", "scenes", "cornell.npz"))
W, H = 1920, 1080
cam = pkg.scenes.default_camera(W, H)
sc = pkg.Scene(sd, device=0)
want, _ = sc.render(cam, W, H)
keep = [torch.empty(3 << 20, dtype=torch.uint8, device="cuda:0") for _ in range(5)]  # (the frames below start mid-segment)
for fmt in ("rgb", "chw", "rgba8"):
    t, _ = sc.render_tensor(cam, W, H, format=fmt)
    got = t.cpu().numpy()
    if fmt == "rgba8":
        assert np.array_equal(got, pkg.rgba8_of(want, W, H)), fmt
    else:
        got = got.transpose(1, 2, 0) if fmt == "chw" else got
        assert np.array_equal(np.ascontiguousarray(got).reshape(-1, 3).view(np.uint32), want.view(np.uint32)), fmt
canvas = torch.zeros((H + 8, 2 * W, 3), dtype=torch.float32, device="cuda:0")  # 52 MB, the frame in its interior
t, _ = sc.render_tensor(cam, W, H, out=canvas[4:4 + H, 100:100 + W])
assert np.array_equal(np.ascontiguousarray(canvas[4:4 + H, 100:100 + W].cpu().numpy()).reshape(-1, 3).view(np.uint32), want.view(np.uint32))
segs = torch.cuda.memory_snapshot()
print("expandable segments:", sum(1 for g in segs if g.get("is_expandable")), "of", len(segs))
print("EXPANDABLE_OK")
"""


def test_render_tensor_with_expandable_segments(pkg):
    """torch's allocator with expandable segments maps its pool in pieces through the virtual-memory API: d_out's check must accept a
    frame that spans pieces (a fresh process: the allocator's mode is fixed when torch first uses the device)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    conf = "expandable_segments:True"
    env = dict(os.environ, PYTORCH_HIP_ALLOC_CONF=conf, PYTORCH_CUDA_ALLOC_CONF=conf, CGRT_ROOT=root)
    r = subprocess.run([sys.executable, "-c", _EXPANDABLE], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "EXPANDABLE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


class _MemLocation(C.Structure):
    _fields_ = [("type", C.c_int), ("id", C.c_int)]


class _AllocProp(C.Structure):  # hipMemAllocationProp
    _fields_ = [("type", C.c_int), ("requestedHandleType", C.c_int), ("location", _MemLocation), ("win32HandleMetaData", C.c_void_p),
                ("compressionType", C.c_ubyte), ("gpuDirectRDMACapable", C.c_ubyte), ("usage", C.c_ushort)]


class _AccessDesc(C.Structure):  # hipMemAccessDesc
    _fields_ = [("location", _MemLocation), ("flags", C.c_int)]


def test_render_device_into_memory_mapped_in_pieces(pkg, scene_data):
    """A frame that spans two physical allocations mapped back to back in one reserved address range (the virtual-memory API, as a
    caching allocator with expandable segments uses it): d_out's check walks the pieces, and the frame lands across the seam."""
    hip = C.CDLL(pkg.LIB_PATH)  # (the runtime libcgrt.so uses)

    def ok(rc, what):
        assert rc == 0, f"{what}: {rc}"

    loc = _MemLocation(1, 0)  # hipMemLocationTypeDevice, device 0
    prop = _AllocProp(type=1, requestedHandleType=0, location=loc)  # hipMemAllocationTypePinned, hipMemHandleTypeNone
    gran = C.c_size_t()
    ok(hip.hipMemGetAllocationGranularity(C.byref(gran), C.byref(prop), 0), "granularity")
    g = gran.value
    W = 1024
    H = -(-3 * g // (2 * W * 12))  # an RGB frame of about 1.5 pieces
    need = W * H * 12
    piece = -(-(-(-need // 2)) // g) * g
    assert piece < need <= 2 * piece
    base = C.c_void_p()
    ok(hip.hipMemAddressReserve(C.byref(base), C.c_size_t(2 * piece), C.c_size_t(0), None, C.c_ulonglong(0)), "reserve")
    handles, mapped = [], []
    try:
        for i in range(2):
            h = C.c_void_p()
            ok(hip.hipMemCreate(C.byref(h), C.c_size_t(piece), C.byref(prop), C.c_ulonglong(0)), "create")
            handles.append(h)
            ok(hip.hipMemMap(C.c_void_p(base.value + i * piece), C.c_size_t(piece), C.c_size_t(0), h, C.c_ulonglong(0)), "map")
            mapped.append(base.value + i * piece)
        acc = _AccessDesc(loc, 3)  # hipMemAccessFlagsProtReadWrite
        ok(hip.hipMemSetAccess(base, C.c_size_t(2 * piece), C.byref(acc), C.c_size_t(1)), "access")
        ok(hip.hipMemset(base, 0, C.c_size_t(2 * piece)), "memset")
        ok(hip.hipDeviceSynchronize(), "sync")
        sc = pkg.Scene(scene_data("cornell"), device=0)
        cam = pkg.scenes.default_camera(W, H)
        want, _ = sc.render(cam, W, H)
        for aa in (False, True):
            want_aa = sc.render_aa(cam, W, H)[0] if aa else want
            st = sc.render_device(cam, W, H, base.value, aa=aa)
            assert st["primary_rays"] == W * H * (4 if aa else 1)
            got = np.empty((W * H, 3), np.float32)
            ok(hip.hipMemcpy(C.c_void_p(got.ctypes.data), base, C.c_size_t(need), 2), "download")  # (default stream: behind the export)
            assert _same_bits(got, want_aa), aa
        print(f"pieces of {piece} bytes (granularity {g}), frame {need} bytes")
    finally:
        hip.hipDeviceSynchronize()
        for p in mapped:
            hip.hipMemUnmap(C.c_void_p(p), C.c_size_t(piece))
        for h in handles:
            hip.hipMemRelease(h)
        hip.hipMemAddressFree(base, C.c_size_t(2 * piece))

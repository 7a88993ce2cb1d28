"""No GPU: the bitwise-reproducible form of the table adjoint (cgrt_surface_grad_repro_workspace, cgrt_interpolate_hits_grad_repro*,
cgrt_surface_*_grad_repro_device; include/cgrt.h).

* Properties of tests/surface_grad_repro_ref.py, the numpy restatement the GPU tests hold the device to: permutation invariance; the
  header's bound gamma(m + 1) * S_abs + (m + 1) * 2^-126 against exact rational sums; exactness where every product and partial sum is
  exact (subnormals included); the non-finite rules; S at the item counts where it changes.
* Through the library on a host-only scene: every CGRT_E_ARG case of the new entries comes before CGRT_E_NO_DEVICE, in the order the
  header states (the twin's checks first, then the workspace's); the workspace size is reported."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import surface_grad_ref as gr
import surface_grad_repro_ref as rr

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_surface_grad_repro_workspace", "cgrt_interpolate_hits_grad_repro", "cgrt_interpolate_hits_grad_repro_device",
           "cgrt_surface_views_grad_repro_device", "cgrt_surface_raycams_grad_repro_device")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the restatement ----
def test_shift_values():
    assert rr.shift(1) == 24 and rr.shift(5461) == 24 and rr.shift(5462) == 23
    assert rr.shift(1 << 20) == 16 and rr.shift(0x7FFFFFFF) == 5
    for n in (1, 5461, 5462, 1 << 20, 0x7FFFFFFF):  # 3 n terms below 2^(24 + S) stay inside int64
        assert (1 << (24 + rr.shift(n))) * 3 * n <= 1 << 62


def _multiset(rng, m, spread, centre):
    e = rng.uniform(centre - spread, centre + spread, m)
    return (np.where(rng.random(m) < 0.5, -1.0, 1.0) * rng.uniform(1.0, 2.0, m) * 2.0 ** e).astype(np.float32)


CASES = [(1, 0, 0), (2, 30, 0), (7, 60, 0), (100, 5, 0), (100, 60, 10), (1000, 20, -20), (5000, 3, 0), (300, 12, -135), (300, 2, -147),
         (64, 20, 90)]


@pytest.mark.parametrize("m,spread,centre", CASES)
def test_permutation_invariance_and_the_bound(m, spread, centre):
    rng = np.random.default_rng(m + spread)
    for trial in range(6):
        x = _multiset(rng, m, spread, centre)
        a = _multiset(rng, 1, spread, centre) if trial % 2 else np.zeros(1, np.float32)
        n = (m, 5462, 1 << 20, 0x7FFFFFFF, 3 * m, m + 1)[trial]
        n = max(n, -(-m // 3))  # (an item contributes at most three times to one element)
        dest = np.zeros(m, np.int64)
        got = rr.accumulate(a, dest, x, n)
        for _ in range(4):
            p = rng.permutation(m)
            assert (_bits(rr.accumulate(a, dest, x[p], n)) == _bits(got)).all(), (m, spread, centre, trial)
        exact = Fraction(float(a[0])) + sum(Fraction(float(v)) for v in x)
        S_abs = Fraction(float(abs(a[0]))) + sum(Fraction(float(abs(v))) for v in x)
        k = m + 1
        lim = Fraction(k, 2**24 - k) * S_abs + k * Fraction(1, 2**126)
        assert np.isfinite(got[0])
        err = abs(Fraction(float(got[0])) - exact)
        assert err <= lim, (m, spread, centre, trial, float(err), float(lim))


def test_other_elements_keep_their_bytes():
    a = np.arange(6, dtype=np.uint32) + np.uint32(0x7FC00001)  # distinct NaN payloads
    got = rr.accumulate(a.view(np.float32), [1, 1, 4], np.asarray([1.0, 2.0, 0.0], np.float32), 3)
    assert (_bits(got)[[0, 2, 3, 5]] == a[[0, 2, 3, 5]]).all()
    assert (_bits(got)[[1, 4]] == rr.QNAN).all(), "a NaN before the call stays NaN, as the one quiet NaN"


@pytest.mark.parametrize("e", [0, -120, -130, -140])
def test_exact_sums_come_out_exact(e):
    """Integers times 2^e with integer partial sums below 2^24: every order of a float sum is exact, and so is the integer form."""
    rng = np.random.default_rng(-e)
    scale = np.float32(2.0**e)
    for m in (1, 3, 64, 1000):
        k = rng.integers(-128, 129, m)
        a_int = int(rng.integers(-8, 9))
        want = np.float32(float((k.sum() + a_int)) * 2.0**e)
        assert float(want) == float(k.sum() + a_int) * 2.0**e, "representable, subnormal or not"
        x = (k.astype(np.float32) * scale).astype(np.float32)
        for n in (m, 1 << 20, 0x7FFFFFFF):
            got = rr.accumulate(np.asarray([a_int * 2.0**e], np.float32), np.zeros(m, np.int64), x, n)
            assert _bits(got)[0] == _bits(want)[0], (e, m, n, got, want)


def test_zero_contributions_count():
    neg0 = np.asarray([-0.0], np.float32)
    got = rr.accumulate(neg0, [0], np.asarray([-0.0], np.float32), 1)
    assert _bits(got)[0] == 0, "fl32(-0 + 0) is +0: the element was written"
    assert _bits(rr.accumulate(neg0, [], np.zeros(0, np.float32), 1))[0] == 0x80000000, "no contribution: not written"


def test_non_finite_rules():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    a = np.asarray([1.5] * 7 + [-np.inf, np.inf], np.float32)
    dest = [0, 0, 1, 1, 2, 2, 2, 3, 4, 5, 7, 8]
    x = np.asarray([inf, 2.0, -inf, 3.0, inf, -inf, 1.0, nan, 7.0, inf, inf, inf], np.float32)
    got = rr.accumulate(a, dest, x, 12)
    assert got[0] == np.inf and got[1] == -np.inf
    assert _bits(got)[2] == rr.QNAN and _bits(got)[3] == rr.QNAN
    assert got[4] == np.float32(8.5) and got[5] == np.inf
    assert _bits(got)[6] == _bits(a)[6], "untouched"
    assert _bits(got)[7] == rr.QNAN, "-inf + inf"
    assert got[8] == np.inf


def test_truncation_of_small_terms():
    """n = 2^20 gives S = 16: a term 17 binades below E keeps its top 23 bits, one 40 binades below contributes nothing."""
    big, n = np.float32(2.0**20), 1 << 20
    assert rr.shift(n) == 16
    one = rr.accumulate(np.zeros(1, np.float32), [0, 0], np.asarray([big, 2.0**-20], np.float32), n)
    assert one[0] == big
    t = rr.terms(np.asarray([big, np.float32(1 + 2.0**-23) * 2.0**3, 2.0**-20], np.float32), [147, 147, 147], 16)
    assert t.tolist() == [1 << 39, (1 << 23 | 1) >> 1, 0]


# ---- the library, host-only ----
def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    assert callable(getattr(pkg.Scene, "surface_grad_repro_workspace", None))


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
_WS = np.zeros(1 << 16, np.uint64)


def _at(a, off=0):
    return C.c_void_p(a.ctypes.data + off)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _nverts(sc):
    return len(np.asarray(sc.sd.pos_nrm).reshape(-1, 6))


def test_workspace_size(pkg, host_scene):
    nverts = _nverts(host_scene)
    for ch in (1, 3, 32, 256):
        b = host_scene.surface_grad_repro_workspace(ch)
        assert b == 12 * nverts * ch and b <= 16 * nverts * ch
    L, out = pkg.lib(), C.c_uint64(7)
    assert L.cgrt_surface_grad_repro_workspace(None, 3, C.byref(out)) == E_ARG
    assert L.cgrt_surface_grad_repro_workspace(host_scene._h, 3, None) == E_ARG
    assert L.cgrt_surface_grad_repro_workspace(host_scene._h, 0, C.byref(out)) == E_ARG and "channels" in _err(pkg)
    assert L.cgrt_surface_grad_repro_workspace(host_scene._h, 257, C.byref(out)) == E_ARG and out.value == 7


def _list(pkg, sc, device, handle="ok", rays=0, hits=0, n=16, gout=0, channels=3, table=0, ws=0, ws_bytes=None):
    """rays / hits / gout / table / ws: a byte offset into the module's arrays, or None for NULL."""
    p = lambda a, off: None if off is None else _at(a, off)  # noqa: E731
    args = [sc._h if handle == "ok" else None, p(_RAYS, rays), p(_HITS, hits), n, p(_GOUT, gout), channels, p(_TABLE, table)]
    L = pkg.lib()
    if not device:
        return L.cgrt_interpolate_hits_grad_repro(*args)
    need = 12 * _nverts(sc) * max(min(channels, 256), 1)
    return L.cgrt_interpolate_hits_grad_repro_device(*args, p(_WS, ws), need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("device", [False, True])
def test_list_argument_checks_and_their_order(pkg, host_scene, device):
    c = lambda **kw: _list(pkg, host_scene, device, **kw)  # noqa: E731
    need = 12 * _nverts(host_scene) * 3
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(n=0) == E_NO_DEVICE and c(n=0x7fffffff, channels=1) == E_NO_DEVICE
    # the twin's checks, in the twin's order
    assert c(handle=None) == E_ARG
    assert c(rays=None) == E_ARG and c(hits=None) == E_ARG and c(gout=None) == E_ARG and c(table=None) == E_ARG
    assert "NULL" in _err(pkg)
    assert c(rays=None, hits=None, gout=None, table=None, ws=None, n=0) == E_NO_DEVICE, "NULL arrays with n == 0 pass the argument checks"
    assert c(n=0x80000000) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(channels=0) == E_ARG and "channels" in _err(pkg)
    assert c(channels=257) == E_ARG and "channels" in _err(pkg)
    assert c(channels=1) == E_NO_DEVICE and c(channels=256) == E_NO_DEVICE
    assert c(n=1 << 30, channels=256) == E_NO_DEVICE, "exactly 2^40 bytes"
    assert c(n=(1 << 30) + 1, channels=256) == E_ARG and "2^40" in _err(pkg)
    for kw in ({"rays": 2}, {"hits": 2}, {"gout": 2}, {"table": 2}):
        assert c(**kw) == (E_ARG if device else E_NO_DEVICE), kw
        assert not device or "aligned" in _err(pkg)
    assert c(handle=None, n=1 << 40, channels=0, rays=2, ws=None) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 40, channels=0, rays=2, ws=None) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(channels=0, rays=2, ws=None) == E_ARG and "channels" in _err(pkg)
    assert c(n=(1 << 30) + 1, channels=256, rays=2, ws=4) == E_ARG and "2^40" in _err(pkg)
    if not device:
        return
    # then the workspace: NULL, 8-byte alignment, size -- all before the host-only scene
    assert c(rays=2, ws=None) == E_ARG and "aligned" in _err(pkg) and "workspace" not in _err(pkg), "the twin's alignment check comes first"
    assert c(ws=None) == E_ARG and "NULL" in _err(pkg)
    assert c(ws=4) == E_ARG and "d_workspace" in _err(pkg) and "8-byte" in _err(pkg)
    assert c(ws=4, ws_bytes=0) == E_ARG and "8-byte" in _err(pkg), "alignment before size"
    assert c(ws_bytes=need - 1) == E_ARG and "workspace_bytes" in _err(pkg)
    assert c(ws_bytes=need) == E_NO_DEVICE and c(ws_bytes=need + 5, ws=8) == E_NO_DEVICE
    assert c(channels=256, ws_bytes=12 * _nverts(host_scene) * 256 - 1) == E_ARG and "workspace_bytes" in _err(pkg)


def _frames(pkg, sc, raycams, handle="ok", cams="ok", nviews=2, W=16, H=16, depth=0, prim=0, gout=0, channels=3, chw=0, table=0, ws=0,
            ws_bytes=None, cam_edit=None):
    if raycams:
        a = pkg.raycam_array([pkg.RayCamera.from_trackball(pkg.scenes.default_camera(16, 16), 16, 16)] * max(nviews, 1))
        if cam_edit:
            a = a.copy()
            cam_edit(a)
    else:
        a = pkg.camera_array(np.stack([pkg.scenes.default_camera(16, 16)] * max(nviews, 1)))
    p = lambda arr, off: None if off is None else _at(arr, off)  # noqa: E731
    f = pkg.lib().cgrt_surface_raycams_grad_repro_device if raycams else pkg.lib().cgrt_surface_views_grad_repro_device
    need = 12 * _nverts(sc) * max(min(channels, 256), 1)
    return f(sc._h if handle == "ok" else None, _at(a) if cams == "ok" else None, nviews, W, H, p(_PLANE, depth), p(_PLANE, prim), p(_GOUT, gout),
             channels, chw, p(_TABLE, table), p(_WS, ws), need if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("raycams", [False, True])
def test_frame_argument_checks_and_their_order(pkg, host_scene, raycams):
    c = lambda **kw: _frames(pkg, host_scene, raycams, **kw)  # noqa: E731
    need = 12 * _nverts(host_scene) * 3
    assert c() == E_NO_DEVICE and c(chw=1) == E_NO_DEVICE
    assert c(handle=None) == E_ARG and c(depth=None) == E_ARG and c(prim=None) == E_ARG
    assert c(gout=None) == E_ARG and "NULL" in _err(pkg)
    assert c(table=None) == E_ARG and "NULL" in _err(pkg)
    assert c(cams=None) == E_ARG and "cams" in _err(pkg)
    assert c(nviews=0) == E_ARG and c(W=0) == E_ARG and c(H=-1) == E_ARG
    assert c(nviews=3, W=1 << 15, H=1 << 15) == E_ARG and "0x7fffffff" in _err(pkg)
    if raycams:
        def nan_origin(a):
            a.view(np.float32).reshape(len(a), -1)[0, 0] = np.nan

        assert c(cam_edit=nan_origin) == E_ARG and "non-finite" in _err(pkg)
    assert c(channels=0) == E_ARG and c(channels=257) == E_ARG and "channels" in _err(pkg)
    assert c(channels=1) == E_NO_DEVICE and c(channels=256) == E_NO_DEVICE
    assert c(nviews=1, W=1 << 15, H=1 << 15, channels=256) == E_NO_DEVICE, "the largest frame there is: exactly 2^40 bytes"
    for kw in ({"depth": 2}, {"prim": 2}, {"gout": 2}, {"table": 2}):
        assert c(**kw) == E_ARG and "aligned" in _err(pkg) and "8-byte" not in _err(pkg), kw
    # the twin's order holds with a bad workspace behind it
    assert c(depth=None, cams=None, channels=0, gout=2, ws=None) == E_ARG and "NULL argument" in _err(pkg)
    assert c(cams=None, channels=0, gout=2, ws=None) == E_ARG and "cams" in _err(pkg)
    assert c(W=0, channels=0, gout=2, ws=None) == E_ARG and "frame size" in _err(pkg)
    assert c(channels=0, gout=2, ws=None) == E_ARG and "channels" in _err(pkg)
    assert c(gout=2, ws=None) == E_ARG and "4-byte" in _err(pkg)
    # then the workspace, before the host-only scene
    assert c(ws=None) == E_ARG and "NULL" in _err(pkg)
    assert c(ws=4) == E_ARG and "8-byte" in _err(pkg)
    assert c(ws=4, ws_bytes=0) == E_ARG and "8-byte" in _err(pkg)
    assert c(ws_bytes=need - 1) == E_ARG and "workspace_bytes" in _err(pkg)
    assert c(ws_bytes=0) == E_ARG and c(ws_bytes=need) == E_NO_DEVICE


def test_numpy_form_checks_its_arrays(pkg, host_scene):
    rays, hits = np.zeros((4, 7), np.float32), np.zeros(4, pkg.HIT_DTYPE)
    with pytest.raises(ValueError):
        host_scene.interpolate_hits_grad(rays, hits, np.zeros((3, 2), np.float32), reproducible=True)
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.interpolate_hits_grad(rays, hits, np.zeros((4, 2), np.float32), reproducible=True)
    assert e.value.code == E_NO_DEVICE


def test_bound_helper_is_the_header_bound():
    assert float(gr.gamma(3)) == 3 * gr.U / (1 - 3 * gr.U)

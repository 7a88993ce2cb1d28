"""No GPU: signed distance and occupancy (cgrt_signed_distance*; include/cgrt.h).

* The entries are exported and the Python methods exist.
* The argument checks come in the documented order, with the documented codes, on a host-only scene, ending in CGRT_E_NO_DEVICE.
* The header's default directions are the package's INSIDE_DIRECTIONS, bit for bit as float32.
* sdf_grid_points is the grid formula in the (nz, ny, nx) order.
* tests/sdf_ref.py -- the definition on the CPU, what the GPU tests hold the device to -- agrees with the analytic box distance on the
  cube (the 4 096 points of test_crossings_gpu.py's cube test, seed 78): within 1e-5 where |sdf| > 1e-3; at most 2 % of the points may be
  left out (measured: 0.17 % left out, 12.6 % inside).

The cube is the closed mesh here.  blob, monkey and dodge, on which tests/test_sdf_gpu.py runs, are OPEN (tests/test_point_scale_cpu.py
asserts it): their tests pin the definition, not geometry; the sign on a curved closed mesh is held to the float64 winding number in
tests/test_point_scale_cpu.py and tests/test_point_scale_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crossings_ref as xr
import sdf_ref

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_signed_distance", "cgrt_signed_distance_device", "cgrt_signed_distance_grid", "cgrt_signed_distance_grid_device",
           "cgrt_debug_sdf_work")
INF = float("inf")


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in ("sdf", "sdf_device", "sdf_tensor", "sdf_grid", "sdf_grid_device", "sdf_grid_tensor", "debug_sdf_work", "inside_tensor",
                 "signed_distance_tensor"):
        assert callable(getattr(pkg.Scene, name, None)), name
    assert callable(pkg.sdf_grid_points)
    assert C.sizeof(pkg.SdfParams) == 4 + 4 + 7 * 3 * 4 and C.sizeof(pkg.Grid) == 36


def test_header_default_directions_are_inside_directions(pkg):
    hdr = open(os.path.join(pkg.INCLUDE_DIR, "cgrt.h")).read()
    m = re.search(r"#define CGRT_SDF_DEFAULT_DIRS\s*\\\n(.*)\n", hdr)
    assert m, "the header states the default directions once, as CGRT_SDF_DEFAULT_DIRS"
    vals = re.findall(r"(-?\d+\.\d+(?:[eE][-+]?\d+)?)f", m.group(1))
    n = int(re.search(r"#define CGRT_SDF_DEFAULT_NDIRS (\d+)", hdr).group(1))
    assert n == 3 and len(vals) == 9
    got = np.array([np.float32(v) for v in vals], np.float32).reshape(3, 3)
    want = np.asarray(pkg.INSIDE_DIRECTIONS, np.float32)
    assert got.shape == want.shape and (got.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 3, 2), (2, 1, 7)])
def test_grid_points(pkg, dims):
    origin, spacing = (-0.3, 0.1, 1.7), (0.1, -0.37, 0.0)
    got = pkg.sdf_grid_points(origin, spacing, dims)
    want = sdf_ref.grid_points(origin, spacing, dims)
    nx, ny, nz = dims
    assert got.dtype == np.float32 and got.shape == (nx * ny * nz, 3)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    g = got.reshape(nz, ny, nx, 3)  # x fastest
    o, sp = np.asarray(origin, np.float32), np.asarray(spacing, np.float32)
    assert g[nz - 1, 0, 0, 2] == o[2] + np.float32(nz - 1) * sp[2] and g[0, ny - 1, 0, 1] == o[1] + np.float32(ny - 1) * sp[1]
    assert g[0, 0, nx - 1, 0] == o[0] + np.float32(nx - 1) * sp[0]
    assert (g[..., 0] == g[0, 0, :, 0]).all() and (g[..., 2] == g[:, 0, 0, 2][:, None, None]).all()


def test_reference_against_the_analytic_box_distance(pkg, orc, scene_data):
    sd = scene_data("cube")
    p = xr.positions(sd)
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    rng = np.random.default_rng(78)
    ext = hi - lo
    pts = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (4096, 3)).astype(np.float32)
    q = pts.astype(np.float64)
    out = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    inside = (out == 0).all(axis=1)
    want = np.where(inside, -np.minimum(q - lo, hi - q).min(axis=1), np.sqrt((out * out).sum(axis=1)))
    keep = np.abs(want) > 1e-3
    got, got_in = sdf_ref.reference(orc, sd, pts, pkg.INSIDE_DIRECTIONS)
    assert got.dtype == np.float32 and got_in.dtype == np.bool_
    print(f"cube: {100.0 * (~keep).mean():.2f} % left out, {100.0 * inside.mean():.1f} % inside, "
          f"largest error {np.abs(got[keep] - want[keep]).max():.2e}")
    assert (~keep).sum() <= 0.02 * len(pts)
    assert inside[keep].any() and (~inside[keep]).any()
    assert (got_in[keep] == inside[keep]).all(), int((got_in[keep] != inside[keep]).sum())
    assert (np.signbit(got) == got_in).all(), "the sign is the vote"
    assert np.abs(got[keep] - want[keep]).max() <= 1e-5
    # the rules beside the search
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], np.float32)
    s, i = sdf_ref.reference(orc, sd, special, pkg.INSIDE_DIRECTIONS)
    assert np.isposinf(s).all() and not i.any()
    s, i = sdf_ref.reference(orc, scene_data("spheres"), pts[:8], pkg.INSIDE_DIRECTIONS)
    assert np.isposinf(s).all() and not i.any()
    s, i = sdf_ref.reference(orc, sd, pts[:256], pkg.INSIDE_DIRECTIONS, max_dist2=0.0)
    assert np.isinf(s).all() and (np.signbit(s) == i).all() and (i == got_in[:256]).all(), "beyond max_dist2: +-inf with the vote's sign"


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


N = 16
_POINTS = np.zeros(N * 3 + 4, np.float32)
_SDF = np.zeros(N + 4, np.float32)
_INSIDE = np.zeros(N + 8, np.uint8)
_WORK = np.zeros(5, np.uint64)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _params(pkg, max_dist2=INF, dirs=None):
    p = pkg.SdfParams()
    p.max_dist2 = max_dist2
    if dirs is not None:
        p.ndirs = len(dirs)
        for j, row in enumerate(dirs[:7]):
            p.dirs[j][:] = list(row)
    return p


def _grid(pkg, dims=(4, 2, 2), origin=(0, 0, 0), spacing=(1, 1, 1)):
    g = pkg.Grid()
    g.origin[:], g.spacing[:], g.dims[:] = list(origin), list(spacing), list(dims)
    return g


def _call(pkg, sc, form, handle="ok", points=0, n=N, params="default", sdf=0, inside=0, grid="default"):
    """points / sdf / inside: a byte offset into the module's arrays, or None for NULL; params / grid: a structure, or None for NULL."""
    p = lambda a, off: None if off is None else C.c_void_p(a.ctypes.data + off)  # noqa: E731
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    prm = _params(pkg) if isinstance(params, str) else params
    prm = None if prm is None else C.byref(prm)
    if form in ("grid", "grid_device"):
        g = _grid(pkg) if isinstance(grid, str) else grid
        g = None if g is None else C.byref(g)
        args = [h, g, prm, p(_SDF, sdf), p(_INSIDE, inside)]
        return L.cgrt_signed_distance_grid_device(*args, None) if form == "grid_device" else L.cgrt_signed_distance_grid(*args)
    if form == "work":
        return L.cgrt_debug_sdf_work(h, p(_POINTS, points), n, prm, 1, p(_WORK, sdf))
    args = [h, p(_POINTS, points), n, prm, p(_SDF, sdf), p(_INSIDE, inside)]
    return L.cgrt_signed_distance_device(*args, None) if form == "device" else L.cgrt_signed_distance(*args)


BAD_PARAMS = (
    ({"max_dist2": float("nan")}, "max_dist2"),
    ({"max_dist2": -1.0}, "max_dist2"),
    ({"dirs": [(1, 0, 0), (0, 1, 0)]}, "ndirs"),
    ({"dirs": [(1, 0, 0)] * 9}, "ndirs"),
    ({"dirs": [(1, 0, 0), (0, 0, 0), (0, 1, 0)]}, "zero"),
    ({"dirs": [(1, 0, 0), (0, 1, 0), (0, float("nan"), 1)]}, "finite"),
    ({"dirs": [(float("inf"), 0, 0)]}, "finite"),
)


@pytest.mark.parametrize("form", ["host", "device", "work"])
def test_argument_checks_of_the_list_entries_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    dev, work = form == "device", form == "work"
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(params=None) == E_NO_DEVICE, "NULL params: all defaults"
    assert c(n=0x7FFFFFFF) == E_NO_DEVICE
    assert c(params=_params(pkg, 0.0, [(1, 2, 3)] * 7)) == E_NO_DEVICE and c(params=_params(pkg, 4.0, [(0, 0, -1e-30)])) == E_NO_DEVICE
    if not work:
        assert c(sdf=None) == E_NO_DEVICE and c(inside=None) == E_NO_DEVICE, "either output may be NULL"
    # 1 - 4
    assert c(handle=None) == E_ARG and "scene" in _err(pkg)
    assert c(points=None) == E_ARG and "NULL" in _err(pkg)
    assert c(sdf=None, inside=None) == E_ARG and "NULL" in _err(pkg)
    assert c(points=None, n=0) == E_NO_DEVICE, "NULL points with n == 0 are allowed"
    assert c(n=0x80000000) == E_ARG and "0x7fffffff" in _err(pkg)
    # 5: the parameters
    for kw, word in BAD_PARAMS:
        assert c(params=_params(pkg, **kw)) == E_ARG and word in _err(pkg), kw
    # 6 (device form): d_points and d_sdf 4-byte aligned; d_inside is bytes
    for kw in ({"points": 2}, {"sdf": 2}):
        if work and "sdf" in kw:
            continue
        assert c(**kw) == (E_ARG if dev else E_NO_DEVICE), kw
        assert not dev or "aligned" in _err(pkg)
    if not work:
        assert c(inside=1) == E_NO_DEVICE
    # the order
    bad = _params(pkg, -1.0)
    assert c(handle=None, points=None, sdf=None, inside=None, n=1 << 40, params=bad) == E_ARG and "scene" in _err(pkg)
    assert c(points=None, sdf=None, inside=None, n=1 << 40, params=bad) == E_ARG and "NULL" in _err(pkg) and "neither" not in _err(pkg)
    assert c(sdf=None, inside=None, n=1 << 40, params=bad) == E_ARG and "neither" in _err(pkg)
    assert c(points=2, n=1 << 40, params=bad) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(points=2, params=bad) == E_ARG and "max_dist2" in _err(pkg)
    assert c(points=2) == (E_ARG if dev else E_NO_DEVICE)


@pytest.mark.parametrize("form", ["grid", "grid_device"])
def test_argument_checks_of_the_grid_entries_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    dev = form == "grid_device"
    assert c() == E_NO_DEVICE and c(params=None) == E_NO_DEVICE
    assert c(sdf=None) == E_NO_DEVICE and c(inside=None) == E_NO_DEVICE
    assert c(grid=_grid(pkg, (1 << 24, 1, 127))) == E_NO_DEVICE and c(grid=_grid(pkg, (1, 0x7FFFFFFF >> 8, 1 << 8))) == E_NO_DEVICE
    assert c(grid=_grid(pkg, spacing=(0.0, -1.0, 1e30))) == E_NO_DEVICE, "zero or negative spacing is allowed"
    assert c(handle=None) == E_ARG and "scene" in _err(pkg)
    assert c(grid=None) == E_ARG and "NULL" in _err(pkg)
    assert c(sdf=None, inside=None) == E_ARG and "neither" in _err(pkg)
    for dims in ((0, 1, 1), (1, 1, 0), ((1 << 24) + 1, 1, 1), (1, 1, 0xFFFFFFFF)):
        assert c(grid=_grid(pkg, dims)) == E_ARG and "2^24" in _err(pkg), dims
    for dims in ((1 << 24, 128, 1), (2048, 1024, 1024), (1 << 24, 1 << 24, 1 << 24)):
        assert c(grid=_grid(pkg, dims)) == E_ARG and "0x7fffffff" in _err(pkg), dims
    assert c(grid=_grid(pkg, origin=(0, float("nan"), 0))) == E_ARG and "finite" in _err(pkg)
    assert c(grid=_grid(pkg, spacing=(float("inf"), 1, 1))) == E_ARG and "finite" in _err(pkg)
    for kw, word in BAD_PARAMS:
        assert c(params=_params(pkg, **kw)) == E_ARG and word in _err(pkg), kw
    assert c(sdf=2) == (E_ARG if dev else E_NO_DEVICE)
    assert not dev or "aligned" in _err(pkg)
    # the order
    bad, big = _params(pkg, -1.0), _grid(pkg, (1 << 24, 1 << 24, 2))
    assert c(handle=None, grid=None, sdf=None, inside=None, params=bad) == E_ARG and "scene" in _err(pkg)
    assert c(grid=None, sdf=None, inside=None, params=bad) == E_ARG and "grid" in _err(pkg)
    assert c(grid=big, sdf=None, inside=None, params=bad) == E_ARG and "neither" in _err(pkg)
    assert c(grid=big, sdf=2, params=bad) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(sdf=2, params=bad) == E_ARG and "max_dist2" in _err(pkg)


def test_numpy_forms_on_a_host_only_scene(pkg, host_scene):
    pts = np.zeros((4, 3), np.float32)
    for f in (host_scene.sdf, host_scene.debug_sdf_work, lambda p: host_scene.sdf(p, want=("inside",)),
              lambda p: host_scene.sdf_grid((0, 0, 0), (1, 1, 1), (2, 2, 2))):
        with pytest.raises(pkg.CgrtError) as e:
            f(pts)
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        host_scene.sdf(np.zeros((4, 2), np.float32))  # (not n x 3)
    with pytest.raises(ValueError):
        host_scene.sdf(pts, directions=[(1, 0, 0), (0, 1, 0)])  # an even count
    with pytest.raises(ValueError):
        host_scene.sdf(pts, want=("distance",))
    for bad in ([(0, 0, 0)], [(1, 0, float("nan"))]):
        with pytest.raises(pkg.CgrtError) as e:
            host_scene.sdf(pts, directions=bad)
        assert e.value.code == E_ARG

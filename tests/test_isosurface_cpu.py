"""No GPU: iso-surfaces (cgrt_isosurface*; include/cgrt.h "Iso-surfaces").

* The five entries are exported, the Python methods exist, CgrtIsoParams is 8 bytes {0, 4}.
* The argument checks come in the documented order on a host-only scene, for the host and the device entries, ending in CGRT_E_NO_DEVICE;
  the workspace size is at most 8 bytes per point + 64 KB, and more than 2^28 points are refused.
* The table derived by rule (tests/isosurface_ref.py, which the GPU tests compare bytes with) equals the one the header prints; the six
  tetrahedra are positively oriented and tile the cell.
* The restatement's properties: the sphere on 6^3 .. 24^3 is closed with Euler characteristic 2 and no unreferenced vertex, its volume
  within 2 % of 4 pi / 3 at 16^3 and 1 % at 24^3 (measured: 1.27 % and 0.54 % under); the torus is closed with characteristic 0; the integer
  field, whose zeros fall on grid points, gives 74 vertices, 144 triangles and volume 32 / 3.
* inside_above on negated data gives the same bytes; scaling the grid by 2^+-20 scales the vertices, scaling values and iso by 2^+-20 changes
  nothing."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import isosurface_ref as iref

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_isosurface_workspace", "cgrt_isosurface_count_device", "cgrt_isosurface_device", "cgrt_isosurface", "cgrt_debug_isosurface_work")
METHODS = ("isosurface", "isosurface_workspace", "isosurface_count_device", "isosurface_device", "isosurface_tensor", "debug_isosurface_work",
           "sdf_isosurface_tensor", "winding_isosurface_tensor")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in METHODS:
        assert callable(getattr(pkg.Scene, name, None)), name
    assert callable(getattr(pkg.scenes, "mesh_scene_data", None))
    assert C.sizeof(pkg.IsoParams) == 8 and [getattr(pkg.IsoParams, k).offset for k in ("iso", "flags")] == [0, 4]
    assert pkg.ISO_INSIDE_ABOVE == 1


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


DIMS = (4, 3, 2)
_VAL = np.zeros(24 + 4, np.float32)
_VERTS = np.zeros(3 * 8 + 4, np.float32)
_TRIS = np.zeros(3 * 8 + 4, np.uint32)
_CNT = np.zeros(4, np.uint64)
_WS = np.zeros(1 << 17, np.uint8)  # (more than the workspace of 24 points; never touched: the scene is host-only)


def _p(a, off):
    return None if off is None else C.c_void_p(a.ctypes.data + off)


def _call(pkg, sc, form, handle="ok", grid="ok", dims=DIMS, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), params="ok", iso=0.0, flags=0,
          values=0, verts=0, vcap=8, tris=0, tcap=8, counts=0, ws=0, ws_bytes=None):
    """form: host / work (host pointers) or dcount / dlist (device).  values / verts / tris / counts / ws: a byte offset into the module's
    arrays, or None for NULL."""
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    g = None
    if grid is not None:
        gs = pkg.Grid()
        gs.origin[:], gs.spacing[:], gs.dims[:] = origin, spacing, dims
        g = C.byref(gs)
    q = None
    if params is not None:
        prm = pkg.IsoParams()
        prm.iso, prm.flags = iso, flags
        q = C.byref(prm)
    if form == "host":
        return L.cgrt_isosurface(h, g, _p(_VAL, values), q, _p(_VERTS, verts), vcap, _p(_TRIS, tris), tcap, _p(_CNT, counts))
    if form == "work":
        return L.cgrt_debug_isosurface_work(h, g, _p(_VAL, values), q, _p(_CNT, counts))
    base = (-_WS.ctypes.data) % 8
    need = C.c_uint64(0)
    if ws_bytes is None:
        gs2 = pkg.Grid()
        gs2.origin[:], gs2.spacing[:], gs2.dims[:] = (0, 0, 0), (1, 1, 1), dims
        if L.cgrt_isosurface_workspace(sc._h, C.byref(gs2), C.byref(need)) != 0:  # (dims beyond the limits: that check comes first anyway)
            gs2.dims[:] = DIMS
            assert L.cgrt_isosurface_workspace(sc._h, C.byref(gs2), C.byref(need)) == 0
        ws_bytes = need.value
    w = (_p(_WS, None if ws is None else base + ws), ws_bytes)
    if form == "dcount":
        return L.cgrt_isosurface_count_device(h, g, _p(_VAL, values), q, _p(_CNT, counts), *w, None)
    assert form == "dlist"
    return L.cgrt_isosurface_device(h, g, _p(_VAL, values), q, _p(_VERTS, verts), vcap, _p(_TRIS, tris), tcap, _p(_CNT, counts), *w, None)


@pytest.mark.parametrize("form", ["host", "work", "dcount", "dlist"])
def test_argument_checks_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    inf, nan = float("inf"), float("nan")
    device, lists = form[0] == "d", form in ("host", "dlist")
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(flags=1) == E_NO_DEVICE and c(iso=-3e38) == E_NO_DEVICE
    assert c(dims=(1, 5, 5)) == E_NO_DEVICE and c(dims=(1 << 24, 16, 1)) == E_NO_DEVICE
    # every later step is broken in each call below: the step under test is the one that is reported
    broken = dict(values=None, counts=None, ws=None)
    # 1. NULL scene, grid or params
    assert c(handle=None, dims=(0, 1, 1), iso=nan, **broken) == E_ARG
    assert c(grid=None, iso=nan, **broken) == E_ARG and "NULL" in pkg.lib().cgrt_last_error().decode()
    assert c(params=None, dims=(0, 1, 1), **broken) == E_ARG and "NULL" in pkg.lib().cgrt_last_error().decode()
    # 2. the grid's limits
    for dims in ((0, 2, 2), (2, (1 << 24) + 1, 1), (1 << 14, 1 << 14, 2), (1 << 24, 1 << 24, 1 << 24)):
        assert c(dims=dims, iso=nan, **broken) == E_ARG and "grid" in pkg.lib().cgrt_last_error().decode(), dims
    assert c(origin=(0.0, inf, 0.0), iso=nan, **broken) == E_ARG and "grid" in pkg.lib().cgrt_last_error().decode()
    assert c(spacing=(nan, 1.0, 1.0), iso=nan, **broken) == E_ARG and "grid" in pkg.lib().cgrt_last_error().decode()
    # 3. iso, flags
    for iso in (nan, inf, -inf):
        assert c(iso=iso, **broken) == E_ARG and "iso" in pkg.lib().cgrt_last_error().decode()
    assert c(flags=2, **broken) == E_ARG and "flags" in pkg.lib().cgrt_last_error().decode()
    # 4. NULL values
    assert c(values=None, counts=None, ws=None) == E_ARG and "values" in pkg.lib().cgrt_last_error().decode()
    # 5. NULL counts2
    assert c(counts=None, verts=None, ws=None) == E_ARG and ("counts2" in pkg.lib().cgrt_last_error().decode() or form == "work")
    if lists:
        # 6. NULL verts or tris with a non-zero capacity
        assert c(verts=None, values=2 if device else 0, ws=None) == E_ARG and "capacity" in pkg.lib().cgrt_last_error().decode()
        assert c(tris=None, values=2 if device else 0, ws=None) == E_ARG and "capacity" in pkg.lib().cgrt_last_error().decode()
        assert c(verts=None, vcap=0, tris=None, tcap=0) == E_NO_DEVICE
    if device:
        # 7. alignments
        for kw in (dict(values=2), dict(counts=4)) + ((dict(verts=2), dict(tris=1)) if lists else ()):
            assert c(ws=None, **kw) == E_ARG and "aligned" in pkg.lib().cgrt_last_error().decode(), kw
        # 8. the workspace
        assert c(ws=None) == E_ARG and "d_workspace" in pkg.lib().cgrt_last_error().decode()
        assert c(ws=4) == E_ARG and "8-byte" in pkg.lib().cgrt_last_error().decode()
        need = pkg.Scene.isosurface_workspace(host_scene, DIMS)
        assert c(ws_bytes=need - 1) == E_ARG and "workspace_bytes" in pkg.lib().cgrt_last_error().decode()
        assert c(ws_bytes=need) == E_NO_DEVICE
    else:
        assert c(values=2) == E_NO_DEVICE, "host pointers need no alignment"


def test_workspace_size(pkg, host_scene):
    for dims in ((1, 1, 1), (2, 2, 2), (17, 9, 5), (96, 64, 64), (256, 256, 256), (1 << 24, 16, 1), (1024, 512, 512)):
        n = dims[0] * dims[1] * dims[2]
        b = host_scene.isosurface_workspace(dims)
        assert 6 * n <= b <= 8 * n + (64 << 10), (dims, b)
    L = pkg.lib()
    for dims in ((1 << 14, 1 << 14, 2), (1025, 512, 512), (0, 1, 1), ((1 << 24) + 1, 1, 1)):
        g = pkg.Grid()
        g.origin[:], g.spacing[:], g.dims[:] = (0, 0, 0), (1, 1, 1), dims
        b = C.c_uint64(0)
        assert L.cgrt_isosurface_workspace(host_scene._h, C.byref(g), C.byref(b)) == E_ARG, dims
    g.dims[:] = (2, 2, 2)
    assert L.cgrt_isosurface_workspace(None, C.byref(g), C.byref(b)) == E_ARG
    assert L.cgrt_isosurface_workspace(host_scene._h, None, C.byref(b)) == E_ARG
    assert L.cgrt_isosurface_workspace(host_scene._h, C.byref(g), None) == E_ARG


# ---- the table and the subdivision ----
def test_rule_derived_table_equals_the_headers():
    text = open(os.path.join(ROOT, "include", "cgrt.h")).read()
    section = text[text.index("/* Iso-surfaces"):]
    section = section[: section.index("*/")]
    printed = iref.parse_header_table(section)
    derived = iref.derive_table()
    assert sorted(printed) == list(range(16))
    for m in range(16):
        assert printed[m] == derived[m], m
    assert [len(derived[m]) for m in range(16)] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    line = "(0,1,3,7) (0,5,1,7) (0,3,2,7) (0,2,6,7) (0,4,5,7) (0,6,4,7)"
    assert line in section and line == " ".join("(" + ",".join(str(c) for c in t) + ")" for t in iref.TETS)


def test_tetrahedra_are_positive_and_tile_the_cell():
    P = iref.CORNERS.astype(np.float64)
    vols = [np.linalg.det(P[list(t)][1:] - P[t[0]]) / 6.0 for t in iref.TETS]
    assert all(v > 0 for v in vols) and abs(sum(vols) - 1.0) < 1e-15
    # each is a chain of corner bit sets 0 < a < b < 7, so the smaller corner of an edge owns it; the six are the six such chains
    chains = set()
    for t in iref.TETS:
        s = sorted(t)
        assert all(s[k] & s[k + 1] == s[k] for k in range(3)), t
        chains.add(tuple(s))
    assert len(chains) == 6
    # a random interior point lies in exactly one (closed) tetrahedron
    rng = np.random.default_rng(5)
    for x in rng.uniform(0.0, 1.0, (200, 3)):
        inside = 0
        for t in iref.TETS:
            lam = np.linalg.solve(np.vstack([P[list(t)].T, np.ones(4)]), np.append(x, 1.0))
            inside += bool((lam > 1e-12).all())
        assert inside == 1


# ---- the restatement's properties ----
@pytest.mark.parametrize("n", [6, 9, 12, 16, 24])
def test_sphere_is_closed(n):
    val, o, sp = iref.field("sphere", (n, n, n))
    verts, tris = iref.isosurface(val, o, sp)
    assert len(tris) > 0 and iref.is_closed(tris)
    assert iref.euler_characteristic(len(verts), tris) == 2 and iref.unreferenced(len(verts), tris) == 0
    vol, exact = iref.signed_volume(verts, tris), 4.0 * math.pi / 3.0
    print(f"sphere {n}^3: {len(verts)} vertices, {len(tris)} triangles, volume {100.0 * (vol / exact - 1.0):+.2f} % of 4 pi / 3")
    assert vol > 0
    if n == 16:
        assert (len(verts), len(tris)) == (2198, 4392) and abs(vol / exact - 1.0) < 0.02
    if n == 24:
        assert (len(verts), len(tris)) == (5150, 10296) and abs(vol / exact - 1.0) < 0.01


def test_torus_is_closed():
    val, o, sp = iref.field("torus", (20, 20, 20), box=1.6)
    verts, tris = iref.isosurface(val, o, sp)
    assert len(tris) > 0 and iref.is_closed(tris) and iref.euler_characteristic(len(verts), tris) == 0


def test_integer_field():
    val, o, sp = iref.integer_field()
    verts, tris, work = iref.isosurface(val, o, sp, want_work=True)
    assert (len(verts), len(tris)) == (74, 144) and work[2:] == (74, 144)
    assert iref.is_closed(tris) and iref.unreferenced(len(verts), tris) == 0
    assert abs(iref.signed_volume(verts, tris) - 32.0 / 3.0) < 1e-6
    # the zeros fall on grid points: several vertices share such a point, and the zero-area triangles between them are kept
    assert len(np.unique(verts, axis=0)) < len(verts)
    p = verts.astype(np.float64)[tris.astype(np.int64)]
    assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any()


@pytest.mark.parametrize("name", ["sphere", "gyroid", "noise"])
def test_inside_above_on_negated_data(name):
    val, o, sp = iref.field(name, (13, 11, 9))
    iso = np.float32(0.125)
    v0, t0 = iref.isosurface(val, o, sp, iso=iso)
    v1, t1 = iref.isosurface(-val, o, sp, iso=-iso, inside_above=True)
    assert v0.tobytes() == v1.tobytes() and t0.tobytes() == t1.tobytes() and len(t0) > 0
    # the flag alone: the same positions where nothing equals iso, every triangle facing the other way
    v2, t2 = iref.isosurface(val, o, sp, iso=iso, inside_above=True)
    assert not (val == iso).any() and v2.tobytes() == v0.tobytes()
    assert sorted(map(tuple, np.sort(t2, 1))) == sorted(map(tuple, np.sort(t0, 1))) and t2.tobytes() != t0.tobytes()
    if name == "sphere":
        assert iref.signed_volume(v0, t0) > 0 > iref.signed_volume(v2, t2)


@pytest.mark.parametrize("k", [-20, 20])
@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_scale_symmetries(name, k):
    val, o, sp = iref.field(name, (12, 10, 9))
    iso, s = np.float32(0.0625), np.float32(2.0**k)
    v0, t0 = iref.isosurface(val, o, sp, iso=iso)
    v1, t1 = iref.isosurface(val, o * s, sp * s, iso=iso)
    assert (v0 * s).tobytes() == v1.tobytes() and t0.tobytes() == t1.tobytes() and len(t0) > 0
    v2, t2 = iref.isosurface(val * s, o, sp, iso=iso * s)
    assert v0.tobytes() == v2.tobytes() and t0.tobytes() == t2.tobytes()


def test_mesh_scene_data(pkg):
    val, o, sp = iref.field("sphere", (10, 10, 10))
    verts, tris = iref.isosurface(val, o, sp)
    sd = pkg.scenes.mesh_scene_data(verts, tris)
    assert sd.pos_nrm.shape == (len(verts), 6) and sd.pos_nrm.dtype == np.float32 and sd.tri.dtype == np.uint32
    assert np.array_equal(sd.tri, tris) and sd.tri_mesh.shape == (len(tris),) and sd.materials.shape == (1, 8)
    n = sd.pos_nrm[:, 3:].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-6)
    # an outward mesh around the origin: the normals point away from it
    assert (np.einsum("ij,ij->i", n, verts.astype(np.float64)) > 0.5).all()
    flat = pkg.scenes.mesh_scene_data([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5]], [[0, 1, 2]])
    assert np.array_equal(flat.pos_nrm[:, 3:], np.tile(np.float32([0, 0, 1]), (4, 1)))
    with pytest.raises(ValueError):
        pkg.scenes.mesh_scene_data(verts, [[0, 1, len(verts)]])
    s = pkg.Scene(sd, device=-1)  # the C-ABI takes it
    s.close()

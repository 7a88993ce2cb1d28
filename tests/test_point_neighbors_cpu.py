"""No GPU: point-set neighbours (cgrt_point_grid_*, cgrt_count_point_neighbors*, cgrt_list_point_neighbors*; include/cgrt.h "Point-set
neighbours").

* The eight entries are exported, the Python methods exist, CgrtPointNeighbor is 8 bytes {0, 4}, CgrtPointQuery 16 bytes {0, 8, 12}.
* The argument checks come in the documented order on a host-only scene, ending in CGRT_E_NO_DEVICE; the workspace size.
* The restatement (tests/point_neighbors_ref.py, which the GPU tests compare bytes with) is held to the header's accuracy bound,
  |d2 / exact - 1| <= (1 + 2^-24)^5 - 1, on seeded clouds in the normal range; its membership equals the float64 membership for every pair
  outside that relative band around r2; the pairs inside the band are counted and are under 1 % of the pairs within 2 r2.
* Fixed cases on an 8^3 lattice of spacing 0.25: at r2 = 0.0625 an interior point has exactly 6 neighbours under skip_same_index, at the
  next float below none; the six-way d2 tie is ordered by index, and k = 3 cuts through it."""
import ctypes as C

import numpy as np
import pytest

import point_neighbors_ref as nref

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_point_grid_workspace", "cgrt_point_grid_build_device", "cgrt_count_point_neighbors", "cgrt_count_point_neighbors_device",
           "cgrt_list_point_neighbors", "cgrt_list_point_neighbors_device", "cgrt_list_point_neighbors_brute", "cgrt_debug_point_neighbor_work")
METHODS = ("point_grid_workspace", "point_grid_build_device", "count_point_neighbors_device", "list_point_neighbors_device",
           "count_point_neighbors", "list_point_neighbors", "nearest_points", "list_point_neighbors_brute", "debug_point_neighbor_work",
           "point_grid_tensor")
GRID_METHODS = ("count", "list", "nearest", "knn")
BAND = (1.0 + 2.0**-24) ** 5 - 1.0


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in METHODS:
        assert callable(getattr(pkg.Scene, name, None)), name
    for name in GRID_METHODS:
        assert callable(getattr(pkg.PointGrid, name, None)), name
    assert C.sizeof(pkg.PointNeighbor) == 8 and [getattr(pkg.PointNeighbor, k).offset for k in ("dist2", "index")] == [0, 4]
    assert C.sizeof(pkg.PointQuery) == 16 and [getattr(pkg.PointQuery, k).offset for k in ("radius2", "max_dist2", "flags")] == [0, 8, 12]
    assert pkg.POINT_NEIGHBOR_DTYPE.itemsize == 8 and pkg.POINT_NEIGHBOR_DTYPE.fields["index"][1] == 4
    assert pkg.POINTS_SKIP_SAME_INDEX == 1


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


N = M = 16
_PTS = np.zeros(N * 3 + 4, np.float32)
_DATA = np.zeros(M * 3 + 4, np.float32)
_RAD = np.zeros(N + 4, np.float32)
_OFF = np.arange(N + 2, dtype=np.uint64)
_OUT = np.zeros(2 * N + 8, np.float32)
_CNT = np.zeros(N + 4, np.uint32)
_GRID = np.zeros(1 << 16, np.uint8)  # (more than the grid of 16 points; never touched: the scene is host-only)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _p(a, off):
    return None if off is None else C.c_void_p(a.ctypes.data + off)


def _query(pkg, query, md, rad, flags):
    if query is None:
        return None
    q = pkg.PointQuery()
    q.radius2, q.max_dist2, q.flags = (None if rad is None else _RAD.ctypes.data + rad), md, flags
    return C.byref(q)


def _call(pkg, sc, form, handle="ok", n=N, m=M, cell=0.5, query="ok", md=1.0, rad=None, flags=0, points=0, data=0, grid=0, grid_bytes=None,
          offsets=None, k=1, out=0, capacity=N, counts=0):
    """form: count / list / brute / work (host) or dcount / dlist (device).  points / data / rad / out / counts / offsets / grid: a byte
    offset into the module's arrays, or None for NULL."""
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    q = _query(pkg, query, md, rad, flags)
    slots = (_p(_OFF, offsets), k, _p(_OUT, out), capacity, _p(_CNT, counts))
    if form in ("dcount", "dlist"):
        base = (-_GRID.ctypes.data) % 8
        need = C.c_uint64(0)
        assert L.cgrt_point_grid_workspace(sc._h, 0, C.byref(need)) == 0
        g = (_p(_GRID, None if grid is None else base + grid), need.value if grid_bytes is None else grid_bytes)
        if form == "dcount":
            return L.cgrt_count_point_neighbors_device(h, *g, _p(_PTS, points), n, q, _p(_CNT, counts), None)
        return L.cgrt_list_point_neighbors_device(h, *g, _p(_PTS, points), n, q, *slots, None)
    lead = (h, _p(_DATA, data), m)
    if form == "count":
        return L.cgrt_count_point_neighbors(*lead, cell, _p(_PTS, points), n, q, _p(_CNT, counts))
    if form == "list":
        return L.cgrt_list_point_neighbors(*lead, cell, _p(_PTS, points), n, q, *slots)
    if form == "brute":
        return L.cgrt_list_point_neighbors_brute(*lead, _p(_PTS, points), n, q, *slots)
    assert form == "work"
    return L.cgrt_debug_point_neighbor_work(*lead, cell, _p(_PTS, points), n, q, k, _p(_OUT, out))


@pytest.mark.parametrize("form", ["count", "list", "brute", "work", "dcount", "dlist"])
def test_argument_checks_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    inf, nan = float("inf"), float("nan")
    device, lists = form[0] == "d", form in ("list", "brute", "dlist")
    grid_form = form in ("count", "list", "work")
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    for md in (0.0, inf, 3e38):
        assert c(md=md) == E_NO_DEVICE, md
    assert c(rad=0) == E_NO_DEVICE and c(flags=1) == E_NO_DEVICE
    assert c(n=0, points=None, data=None, out=None, counts=None, grid=None) == E_NO_DEVICE, "n == 0 needs no array"
    if not device:
        assert c(m=0, data=None) == E_NO_DEVICE, "no data point needs no data"
    # every check with every later one failing too: the earlier one is reported
    later = dict(n=1 << 31, m=1 << 31, cell=nan, md=nan, flags=2, k=0, capacity=1 << 40)
    assert c(handle=None, points=None, **later) == E_ARG and "scene or query" in _err(pkg)
    assert c(query=None, points=None, **later) == E_ARG and "scene or query" in _err(pkg)
    assert c(points=None, **later) == E_ARG and "NULL" in _err(pkg)
    result = dict(counts=None) if form in ("count", "dcount") else dict(out=None)
    assert c(**result, **later) == E_ARG and "NULL" in _err(pkg)
    assert c(**(dict(grid=None) if device else dict(data=None)), **later) == E_ARG and "NULL" in _err(pkg)
    assert c(**later) == E_ARG and "too many queries" in _err(pkg)
    del later["n"]
    if not device:
        assert c(**later) == E_ARG and "too many data" in _err(pkg)
    del later["m"]
    if grid_form:
        for cell in (nan, 0.0, -1.0, inf):
            later["cell"] = cell
            assert c(**later) == E_ARG and "cell" in _err(pkg), cell
    del later["cell"]
    for md in (nan, -1.0, -inf):
        later["md"] = md
        assert c(**later) == E_ARG and "max_dist2" in _err(pkg), md
    assert c(md=nan, rad=0) == E_ARG and "max_dist2" in _err(pkg), "the scalar is checked also where radius2 is given"
    del later["md"]
    assert c(**later) == E_ARG and "flags" in _err(pkg)
    del later["flags"]
    if lists:
        assert c(**later) == E_ARG and "exactly one" in _err(pkg)
        assert c(offsets=0, k=2, capacity=1 << 40) == E_ARG and "exactly one" in _err(pkg)
        assert c(capacity=1 << 40) == E_ARG and "2^37" in _err(pkg)
        assert c(k=2, capacity=2 * N - 1) == E_ARG and "exceed capacity" in _err(pkg)
        if not device:
            assert c(offsets=8, k=0) == E_ARG and "start at 0" in _err(pkg)
            assert c(offsets=0, k=0, capacity=N - 1) == E_ARG and "beyond capacity" in _err(pkg)
            assert c(offsets=0, k=0) == E_NO_DEVICE
        else:
            assert c(offsets=4, k=0) == E_ARG and "aligned" in _err(pkg)
            assert c(out=2) == E_ARG and "aligned" in _err(pkg)
    if device:
        assert c(points=2) == E_ARG and "aligned" in _err(pkg)
        assert c(rad=2) == E_ARG and "aligned" in _err(pkg)
        assert c(grid=4) == E_ARG and "aligned" in _err(pkg)
        need = host_scene.point_grid_workspace(0)
        assert c(grid_bytes=need - 1) == E_ARG and "grid_bytes" in _err(pkg)
        assert c(grid=4, grid_bytes=0) == E_ARG and "aligned" in _err(pkg), "alignment comes before the size"
    else:
        assert c(points=2, data=2, rad=2) == E_NO_DEVICE, "host pointers need no alignment"


def test_build_checks_and_workspace_size(pkg, host_scene):
    L = pkg.lib()
    b = C.c_uint64(0)
    assert L.cgrt_point_grid_workspace(None, 1, C.byref(b)) == E_ARG and L.cgrt_point_grid_workspace(host_scene._h, 1, None) == E_ARG
    assert L.cgrt_point_grid_workspace(host_scene._h, 1 << 31, C.byref(b)) == E_ARG
    sizes = [host_scene.point_grid_workspace(m) for m in (0, 1, 1000, 1 << 20, 0x7FFFFFFF)]
    assert sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes)
    assert 32 * (1 << 20) <= sizes[3] <= 33 * (1 << 20), "24 bytes per point and 8 per bucket"
    base = (-_GRID.ctypes.data) % 8
    need = host_scene.point_grid_workspace(M)

    def build(handle="ok", data=0, m=M, cell=0.5, grid=0, grid_bytes=need):
        return L.cgrt_point_grid_build_device(host_scene._h if handle == "ok" else None, _p(_DATA, data), m, cell,
                                              _p(_GRID, None if grid is None else base + grid), grid_bytes, None)

    assert build() == E_NO_DEVICE and build(m=0, data=None, grid_bytes=host_scene.point_grid_workspace(0)) == E_NO_DEVICE
    later = dict(m=1 << 31, cell=float("nan"), grid_bytes=0)
    assert build(handle=None, data=None, **later) == E_ARG and "scene" in _err(pkg)
    assert build(data=None, **later) == E_ARG and "NULL" in _err(pkg)
    assert build(grid=None, **later) == E_ARG and "NULL" in _err(pkg)
    assert build(**later) == E_ARG and "too many" in _err(pkg)
    for cell in (float("nan"), 0.0, -2.0, float("inf")):
        assert build(cell=cell, data=2, grid_bytes=0) == E_ARG and "cell" in _err(pkg), cell
    assert build(data=2, grid_bytes=0) == E_ARG and "aligned" in _err(pkg)
    assert build(grid=4, grid_bytes=0) == E_ARG and "aligned" in _err(pkg)
    assert build(grid_bytes=need - 1) == E_ARG and "grid_bytes" in _err(pkg)


# ---- the restatement against float64 ----
def _cloud(rng, n, scale=1.0, offset=0.0):
    return (rng.random((n, 3)) * scale + offset).astype(np.float32)


@pytest.mark.parametrize("seed, scale, offset, r", [(1, 1.0, 0.0, 0.1), (2, 1.0, 0.0, 0.3), (3, 2.0**-20, 0.0, 0.15 * 2.0**-20),
                                                     (4, 2.0**20, 0.0, 0.1 * 2.0**20), (5, 1.0, 100.0, 0.2), (6, 16.0, -8.0, 2.5)])
def test_restatement_meets_the_accuracy_bound(seed, scale, offset, r):
    rng = np.random.default_rng(seed)
    data, pts = _cloud(rng, 700, scale, offset), _cloud(rng, 300, scale, offset)
    r2 = np.float32(r * r)
    d2 = nref.d2_matrix(pts, data)
    exact = nref.exact_d2(pts, data)
    assert exact.min() > 0 and float(np.float32(exact.min())) > 2.0**-100, "the normal range: no subnormal intermediate"
    rel = np.abs(d2.astype(np.float64) / exact - 1.0)
    print(f"largest relative error of d2: {rel.max() / 2.0**-24:.3f} * 2^-24 (bound {BAND / 2.0**-24:.7f} * 2^-24)")
    assert rel.max() <= BAND
    mem, _ = nref.members(pts, data, max_dist2=r2, d2=d2)
    want = exact <= float(r2)
    band = np.abs(exact / float(r2) - 1.0) <= BAND
    assert np.array_equal(mem[~band], want[~band]), "membership differs from float64 outside the band"
    near = int((exact <= 2.0 * float(r2)).sum())
    print(f"pairs inside the band: {int(band.sum())} of {near} within 2 r2; of those, membership differs for {int((mem != want).sum())}")
    assert near > 1000 and band.sum() < 0.01 * near


# ---- the lattice ----
def test_lattice_case():
    p = nref.lattice_case()
    assert len(p) == 512
    interior = ((p > 0) & (p < 1.75)).all(1)
    r2 = np.float32(0.0625)
    rec, counts = nref.neighbors(p, p, max_dist2=r2, skip_same_index=True, k=8)
    assert interior.sum() == 216 and (counts[interior] == 6).all() and counts.sum() == 2 * 3 * 7 * 64
    rec0, counts0 = nref.neighbors(p, p, max_dist2=r2, k=8)
    assert (counts0 == counts + 1).all() and (rec0["index"][:, 0] == np.arange(512)).all() and (rec0["dist2"][:, 0] == 0).all()
    below = np.nextafter(r2, np.float32(0))
    _, cb = nref.neighbors(p, p, max_dist2=below, skip_same_index=True, k=1)
    assert cb.sum() == 0, "non-strict at r2, nothing at the next float below"
    i = int(np.flatnonzero(interior)[0])  # (1, 1, 1): index 73, neighbours at +-64, +-8, +-1
    assert i == 73
    six = [i - 64, i - 8, i - 1, i + 1, i + 8, i + 64]
    assert list(rec["index"][i, :6]) == six and (rec["dist2"][i, :6] == r2).all() and (rec["index"][i, 6:] == nref.NO_PRIM).all()
    assert np.isposinf(rec["dist2"][i, 6:]).all()
    rec3, c3 = nref.neighbors(p, p, max_dist2=r2, skip_same_index=True, k=3)
    assert list(rec3["index"][i]) == six[:3] and c3[i] == 6, "k = 3 cuts through the tie: the three smallest indices"
    off, full, cf = nref.neighbors(p, p, max_dist2=r2, skip_same_index=True)
    assert off[-1] == counts.sum() and list(full["index"][off[i] : off[i + 1]]) == six and np.array_equal(cf, counts)

"""No GPU: neighbour queries (cgrt_count_neighbors*, cgrt_list_neighbors*; include/cgrt.h "Neighbour queries").

* tests/neighbors_ref.py -- the numpy float32 restatement the GPU tests hold the device to, byte for byte -- against the float64 referee
  closest_ref.dist64, on closest_ref.mixed_queries(sd, 1024, 11) with radii of 0.05 and 0.1 of the scene's extent.  With R the radius
  (the square root, in float64, of the float32 r2 the restatement is given) and D64 the referee's distance, membership must agree on
  EVERY (query, triangle) pair with |D64 - R| > 5.66 * 2^-24 * max(1, |p|inf, S) -- the accuracy bound of dist2 (include/cgrt.h
  "Closest-point queries", Envelope) -- and the pairs inside that band are classed and counted: at most 1e-4 of the pairs.  Measured
  on the CPU, per radius: 5 pairs of 991 232 inside the band on monkey, 0 on the other scenes; no disagreement outside the band.
* The (dist2, prim_id) order and the slot rule of the restatement on hand-made ties (cube vertices: up to 6 triangles at dist2 == 0),
  with clamped, decreasing and short slots.
* The entries are exported and check their arguments in the documented order on a host-only scene."""
import ctypes as C

import numpy as np
import pytest

import closest_ref as cr
import neighbors_ref as nr

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_count_neighbors", "cgrt_count_neighbors_device", "cgrt_list_neighbors", "cgrt_list_neighbors_device",
           "cgrt_list_neighbors_brute", "cgrt_debug_neighbor_work")
SCENES = ("triangle", "cube", "cornell", "monkey", "blob")
K = 5.66  # include/cgrt.h: sqrt(dist2) is within K * 2^-24 * max(1, |p|inf, S) of the float64 distance
INF = float("inf")

_d64 = {}


def _referee(scene_data, name):
    if name not in _d64:
        sd = scene_data(name)
        q = cr.mixed_queries(sd, 1024, 11)
        _d64[name] = (sd, q, cr.dist64(sd, q))
    return _d64[name]


@pytest.mark.parametrize("frac", [0.05, 0.1])
@pytest.mark.parametrize("name", SCENES)
def test_restatement_against_float64(scene_data, name, frac):
    sd, q, D = _referee(scene_data, name)
    r2 = np.float32(np.float32(frac * nr.extent(sd)) ** 2)
    R = np.sqrt(np.float64(r2))
    member = np.zeros(D.shape, bool)
    for s, _, ok in nr.membership(sd, q, nr.bounds(len(q), None, r2)):
        member[s : s + len(ok)] = ok
    finite = np.isfinite(q).all(axis=1)
    assert (~finite).sum() == 2 and not member[~finite].any(), "the NaN and the inf point have no neighbours"
    scale = np.maximum(1.0, np.maximum(np.abs(q.astype(np.float64)).max(axis=1), cr.scene_scale(sd)))
    band = K * 2.0 ** -24 * scale
    with np.errstate(invalid="ignore"):
        inside = np.abs(D - R) <= band[:, None]
        want = D <= R
    clear = finite[:, None] & ~inside
    wrong = clear & (member != want)
    pairs = D.size
    in_band = int((inside & finite[:, None]).sum())
    print(f"{name}, radius {frac} of the extent: {pairs} pairs, {int(member.sum())} memberships, {in_band} pairs inside the band "
          f"(of which {int((inside & finite[:, None] & (member != want)).sum())} differ), {int(wrong.sum())} disagreements outside it")
    assert not wrong.any(), (name, frac, np.argwhere(wrong)[:4])
    assert in_band <= 1e-4 * pairs, (name, frac, in_band, pairs)
    if name != "triangle":
        assert member.any() and not member[finite].all(), "the radius separates"


def _cube(scene_data):
    sd = scene_data("cube")
    a, b, c = cr.tri_verts(sd)
    corner = a[0].copy()
    return sd, a, b, c, corner


def test_order_on_ties(scene_data):
    sd, a, b, c, corner = _cube(scene_data)
    sharing = np.flatnonzero((a == corner).all(1) | (b == corner).all(1) | (c == corner).all(1))
    assert 3 <= len(sharing) <= 6
    off, rec = nr.neighbors(sd, corner[None, :], None, 0.0)
    assert off.tolist() == [0, len(sharing)]
    assert (rec["dist2"] == 0).all() and rec["prim_id"].tolist() == sorted(sharing.tolist()), "equal dist2: ascending prim_id"
    # unbounded: every triangle, by dist2 and within equal dist2 by prim_id
    off, rec = nr.neighbors(sd, corner[None, :])
    assert off[1] == sd.ntris and sorted(rec["prim_id"].tolist()) == list(range(sd.ntris))
    d, p = rec["dist2"], rec["prim_id"].astype(np.int64)
    assert ((d[:-1] < d[1:]) | ((d[:-1] == d[1:]) & (p[:-1] < p[1:]))).all(), "a strict total order"
    _, d2, _, _, _ = cr.closest_tri32(corner[None, :], a, b, c)
    assert (d2[p].view(np.uint32) == d.view(np.uint32)).all(), "dist2 is closest_points' dist2"


def test_membership_edge_cases(scene_data):
    sd, a, b, c, corner = _cube(scene_data)
    pts = np.stack([corner] * 7)
    pts[5, 0] = np.nan
    pts[6, 1] = np.inf
    radii = np.array([0.0, -0.0, np.nan, -1.0, np.inf, np.inf, 1.0], np.float32)
    off, rec = nr.neighbors(sd, pts, radii)
    counts = np.diff(off)
    tied = counts[0]
    assert tied >= 3 and counts[1] == tied, "r2 = 0 (and -0: `r2 >= 0` is true) accepts dist2 == 0"
    assert counts[2] == 0 and counts[3] == 0, "a NaN and a negative radius: no neighbours"
    assert counts[4] == sd.ntris, "+inf: unbounded"
    assert counts[5] == 0 and counts[6] == 0, "a non-finite point: no neighbours"
    # the scalar bound where there are no radii
    assert np.diff(nr.neighbors(sd, pts[:1], None, 0.0)[0]).tolist() == [tied]


def test_slot_rule(scene_data):
    sd, a, b, c, corner = _cube(scene_data)
    far = (corner + np.float32(100.0)).astype(np.float32)
    pts = np.stack([corner, far, corner, corner])
    full = nr.neighbors(sd, pts, np.array([0.0, 0.0, 0.0, np.inf], np.float32))
    counts = np.diff(full[0]).tolist()
    tied = counts[0]
    assert counts == [tied, 0, tied, sd.ntris]
    first = full[1][:tied]
    # k slots: shorter than, equal to and longer than the count
    for k in (1, 2, tied, tied + 2):
        got = nr.nearest(full, k)
        assert got.shape == (4, k)
        m = min(k, tied)
        assert nr.same(got[0, :m], first[:m]) and (got[0, m:] == nr.UNUSED).all()
        assert (got[1] == nr.UNUSED).all(), "no neighbours: an all-unused slot"
        assert nr.same(got[3, : min(k, sd.ntris)], full[1][full[0][3] : full[0][3] + min(k, sd.ntris)])
    # offsets: a slot that the capacity cuts, a decreasing pair that starts beyond it (empty), a plain slot, an empty one; the records
    # no slot owns keep their bytes
    mark = np.array([(-7.0, 7)], nr.NEIGHBOR_DTYPE)[0]
    got = nr.fill_slots(full, np.full(6, mark, nr.NEIGHBOR_DTYPE), offsets=np.array([4, 7, 1, 3, 3], np.uint64))
    assert nr.same(got[4:6], first[:2]), "query 0 owns [4, 7), cut to [4, 6)"
    assert nr.same(got[1:3], first[:2]), "query 2 owns [1, 3): the first two of its ties"
    assert got[0] == mark and got[3] == mark, "query 1 owns [7, 1) and query 3 [3, 3): nothing; nothing outside the slots"
    got = nr.fill_slots(full, np.full(tied + 3, mark, nr.NEIGHBOR_DTYPE), offsets=np.array([0, tied + 2, tied + 3, tied + 3, tied + 3], np.uint64))
    assert nr.same(got[:tied], first) and (got[tied : tied + 2] == nr.UNUSED).all() and got[tied + 2] == nr.UNUSED, "short lists are padded"


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in ("count_neighbors", "list_neighbors", "nearest_triangles", "list_neighbors_brute", "debug_neighbor_work",
                 "count_neighbors_device", "list_neighbors_device", "count_neighbors_tensor", "list_neighbors_tensor",
                 "nearest_triangles_tensor"):
        assert callable(getattr(pkg.Scene, name, None)), name
    assert pkg.NEIGHBOR_DTYPE == nr.NEIGHBOR_DTYPE and pkg.NEIGHBOR_DTYPE.itemsize == 8


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_N = 16
_POINTS = np.zeros(_N * 3 + 4, np.float32)
_RADII = np.zeros(_N + 4, np.float32)
_OUT = np.zeros(2 * 4 * _N + 4, np.float32)
_COUNTS = np.zeros(_N + 4, np.uint32)
_WORK = np.zeros(4, np.uint64)
_OFFSETS = np.zeros(_N + 3, np.uint64)  # all zero: valid (every slot empty)
_OFF_BAD_START = np.concatenate([[1], np.ones(_N + 1)]).astype(np.uint64)
_OFF_DECREASING = np.concatenate([[0, 2, 1], np.full(_N - 1, 2)]).astype(np.uint64)
_OFF_LONG = np.concatenate([[0], np.full(_N + 1, 65)]).astype(np.uint64)
_OFFS = {"ok": _OFFSETS, "bad_start": _OFF_BAD_START, "decreasing": _OFF_DECREASING, "long": _OFF_LONG}
FORMS = ("count", "count_device", "list", "list_device", "brute", "work")
LISTS = ("list", "list_device", "brute")


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _call(pkg, sc, form, handle="ok", points=0, n=_N, radius2=None, max_dist2=np.inf, offsets=None, offsets_at=0, k=None, out=0, capacity=64,
          counts=0):
    """points / radius2 / out / counts / offsets_at: a byte offset into the module's arrays, or None for NULL; offsets: a key of _OFFS
    or None (then 4 records per query unless k says otherwise)."""
    p = lambda a, off: None if off is None else C.c_void_p(a.ctypes.data + off)  # noqa: E731
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    off = None if offsets is None else p(_OFFS[offsets], offsets_at)
    head = [h, p(_POINTS, points), n, p(_RADII, radius2), float(max_dist2)]
    if form == "count":
        return L.cgrt_count_neighbors(*head, p(_COUNTS, out))
    if form == "count_device":
        return L.cgrt_count_neighbors_device(*head, p(_COUNTS, out), None)
    if form == "work":
        return L.cgrt_debug_neighbor_work(*head, 0, p(_WORK, out))
    k = (0 if offsets is not None else 4) if k is None else k
    tail = [off, k, p(_OUT, out), capacity, p(_COUNTS, counts)]
    if form == "list":
        return L.cgrt_list_neighbors(*head, *tail)
    if form == "brute":
        return L.cgrt_list_neighbors_brute(*head, *tail)
    return L.cgrt_list_neighbors_device(*head, *tail, None)


@pytest.mark.parametrize("form", FORMS)
def test_argument_checks_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    device, lst = form.endswith("_device"), form in LISTS
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(n=0x7fffffff, capacity=1 << 37) == E_NO_DEVICE and c(max_dist2=0.0) == E_NO_DEVICE and c(radius2=0) == E_NO_DEVICE
    # rule 1: NULL scene
    assert c(handle=None) == E_ARG and "scene" in _err(pkg)
    # rule 2: NULL points or result with n > 0
    assert c(points=None) == E_ARG and "NULL" in _err(pkg)
    assert c(out=None) == E_ARG and "NULL" in _err(pkg)
    assert c(points=None, out=None, n=0) == E_NO_DEVICE, "NULL arrays with n == 0 are allowed"
    if lst:
        assert c(counts=None) == E_NO_DEVICE, "counts may be NULL in the list calls"
    # rule 3: n > 0x7fffffff
    assert c(n=0x80000000) == E_ARG and "0x7fffffff" in _err(pkg)
    # rule 4: max_dist2 NaN or negative, also where per-query radii are given
    for bad in (np.nan, -1.0, -np.inf):
        assert c(max_dist2=bad) == E_ARG and "max_dist2" in _err(pkg)
        assert c(max_dist2=bad, radius2=0) == E_ARG and "max_dist2" in _err(pkg)
    if lst:
        # rule 5: both or neither of offsets and k > 0
        assert c(k=0) == E_ARG and "exactly one" in _err(pkg)
        assert c(offsets="ok", k=3) == E_ARG and "exactly one" in _err(pkg)
        assert c(offsets="ok") == E_NO_DEVICE
        # rule 6: capacity above 2^37
        assert c(capacity=(1 << 37) + 1) == E_ARG and "2^37" in _err(pkg)
        # rule 7: n * k > capacity
        assert c(capacity=63) == E_ARG and "exceed capacity" in _err(pkg)
        assert c(k=0xffffffff, n=0x7fffffff, capacity=1 << 37) == E_ARG and "exceed capacity" in _err(pkg)
        # rule 8 (host list calls): the offsets
        for key, word in (("bad_start", "start at 0"), ("decreasing", "decrease"), ("long", "beyond capacity")):
            assert c(offsets=key) == (E_NO_DEVICE if device else E_ARG), (key, "the device form never reads the offsets on the host")
            assert device or word in _err(pkg)
        assert c(offsets="long", capacity=65) == E_NO_DEVICE
    # rule 9 (device forms): every pointer aligned to its element
    misaligned = [{"points": 2}, {"out": 2}, {"radius2": 2}] + ([{"counts": 2}, {"offsets": "ok", "offsets_at": 4}] if lst else [])
    for kw in misaligned:
        assert c(**kw) == (E_ARG if device else E_NO_DEVICE), kw
        assert not device or "aligned" in _err(pkg)
    # the order
    worst = dict(points=None, n=1 << 40, max_dist2=np.nan, out=2)
    if lst:
        worst.update(k=0, capacity=(1 << 37) + 1)
    assert c(handle=None, **worst) == E_ARG and "scene" in _err(pkg)
    assert c(**worst) == E_ARG and "NULL" in _err(pkg)
    del worst["points"]
    assert c(**worst) == E_ARG and "0x7fffffff" in _err(pkg)
    worst["n"] = _N
    assert c(**worst) == E_ARG and "max_dist2" in _err(pkg)
    del worst["max_dist2"]
    if lst:
        assert c(**worst) == E_ARG and "exactly one" in _err(pkg)
        worst["k"] = 5
        assert c(**worst) == E_ARG and "2^37" in _err(pkg)
        worst["capacity"] = 64
        assert c(**worst) == E_ARG and "exceed capacity" in _err(pkg)
        worst["k"] = 4
        if not device:
            assert c(offsets="long", out=2) == E_ARG and "beyond capacity" in _err(pkg)
    assert c(**worst) == (E_ARG if device else E_NO_DEVICE)


def test_work_entry_with_k_checks_its_slots(pkg, host_scene):
    L = pkg.lib()
    h, p, w = host_scene._h, C.c_void_p(_POINTS.ctypes.data), C.c_void_p(_WORK.ctypes.data)
    assert L.cgrt_debug_neighbor_work(h, p, _N, None, np.inf, 8, w) == E_NO_DEVICE
    assert L.cgrt_debug_neighbor_work(h, p, 0x7fffffff, None, np.inf, 0xffffffff, w) == E_ARG and "2^37" in _err(pkg)


def test_numpy_forms_on_a_host_only_scene(pkg, host_scene):
    q = np.zeros((4, 3), np.float32)
    for f in (host_scene.count_neighbors, host_scene.list_neighbors, host_scene.list_neighbors_brute, host_scene.debug_neighbor_work,
              lambda x: host_scene.nearest_triangles(x, 3)):
        with pytest.raises(pkg.CgrtError) as e:
            f(q)
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        host_scene.count_neighbors(np.zeros((4, 2), np.float32))  # (not n x 3)
    with pytest.raises(ValueError):
        host_scene.count_neighbors(q, radius2=np.zeros(3, np.float32))  # (not one radius per point)
    with pytest.raises(ValueError):
        host_scene.nearest_triangles(q, 0)

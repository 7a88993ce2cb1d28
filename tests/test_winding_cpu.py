"""No GPU: winding numbers (cgrt_winding_numbers*; include/cgrt.h "Winding numbers").

* The entries are exported and the Python methods exist.
* The argument checks come in the documented order, with the documented codes, on a host-only scene, ending in CGRT_E_NO_DEVICE.
* The cluster tree of Scene.debug_winding_tree (it builds on a host-only scene) on cube, blob, dodge, the 5 000-triangle dragon and the
  first k triangles of blob: the level counts; EXACTLY, every vertex of every record of a cluster has an f32-evaluated squared distance
  to its centre <= r2; a cluster's area vector is the float64 sum of its records' within 8 * 2^-24 * sum |area vector|, and a parent's
  the sum of its children's within the same bound; the centre is the area-weighted mean of the centroids to f32 rounding.
* Accuracy of the tree form (tests/winding_ref.py walk in float64 on the real tree) against scale_ref.winding64 at beta = 2, 3, 4, +inf on
  sign_queries(sd, 385, 11).  The table is printed (DESIGN.md 5.25 carries a copy).  beta = +inf is the same sum (1e-12); at beta = 2 no
  verdict |w| > 0.5 differs from the truth outside the band ||w64| - 0.5| < 0.05, which may hold 2 % of the points at most; the largest
  error does not grow from beta = 2 to 3 to 4.  No error bound for a finite beta is fixed in advance.
* On the closed fixtures (cube, dragon) the verdict at beta = 2 equals sdf_ref's `inside` at every point farther than 1e-4 extents from
  the surface."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import closest_ref as cr
import scale_ref as sr
import sdf_ref
import winding_ref as wr

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_winding_numbers", "cgrt_winding_numbers_device", "cgrt_winding_numbers_grid", "cgrt_winding_numbers_grid_device",
           "cgrt_winding_numbers_brute", "cgrt_debug_winding_work", "cgrt_debug_get_winding_tree")
METHODS = ("winding_numbers", "winding_numbers_device", "winding_numbers_tensor", "winding_numbers_brute", "winding_grid",
           "winding_grid_device", "winding_grid_tensor", "debug_winding_work", "debug_winding_tree", "inside_winding_tensor",
           "signed_distance_winding_tensor")
INF = float("inf")
TRUNCATIONS = (1, 7, 8, 9, 63, 64, 65, 512, 513)


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in METHODS:
        assert callable(getattr(pkg.Scene, name, None)), name
    assert C.sizeof(pkg.WindingParams) == 8
    for name in ("sdf_tensor", "signed_distance_tensor", "inside_tensor"):
        assert callable(getattr(pkg.Scene, name, None)), name


def truncated(sd, k):
    """The scene's first k triangles."""
    tri = np.asarray(sd.tri).reshape(-1, 3)
    return dataclasses.replace(sd, tri=tri[:k].copy(), tri_mesh=np.asarray(sd.tri_mesh)[:k].copy(), name=f"{sd.name}[:{k}]")


def _scene(pkg, scene_data, name):
    if name == "dragon":
        return pkg.scenes.make_dragon(5000)
    if name.startswith("blob:"):
        return truncated(scene_data("blob"), int(name[5:]))
    return scene_data(name)


# ---- the argument checks, on a host-only scene ----
@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


N = 16
_POINTS = np.zeros(N * 3 + 4, np.float32)
_W = np.zeros(N + 4, np.float32)
_INSIDE = np.zeros(N + 8, np.uint8)
_WORK = np.zeros(3, np.uint64)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _params(pkg, beta=2.0, threshold=0.5):
    p = pkg.WindingParams()
    p.beta, p.threshold = beta, threshold
    return p


def _grid(pkg, dims=(4, 2, 2), origin=(0, 0, 0), spacing=(1, 1, 1)):
    g = pkg.Grid()
    g.origin[:], g.spacing[:], g.dims[:] = list(origin), list(spacing), list(dims)
    return g


def _call(pkg, sc, form, handle="ok", points=0, n=N, params="default", w=0, inside=0, grid="default"):
    """points / w / inside: a byte offset into the module's arrays, or None for NULL; params / grid: a structure, or None for NULL."""
    p = lambda a, off: None if off is None else C.c_void_p(a.ctypes.data + off)  # noqa: E731
    L = pkg.lib()
    h = sc._h if handle == "ok" else None
    prm = _params(pkg) if isinstance(params, str) else params
    prm = None if prm is None else C.byref(prm)
    if form in ("grid", "grid_device"):
        g = _grid(pkg) if isinstance(grid, str) else grid
        g = None if g is None else C.byref(g)
        args = [h, g, prm, p(_W, w), p(_INSIDE, inside)]
        return L.cgrt_winding_numbers_grid_device(*args, None) if form == "grid_device" else L.cgrt_winding_numbers_grid(*args)
    if form == "work":
        return L.cgrt_debug_winding_work(h, p(_POINTS, points), n, prm, p(_WORK, w))
    args = [h, p(_POINTS, points), n, prm, p(_W, w), p(_INSIDE, inside)]
    if form == "device":
        return L.cgrt_winding_numbers_device(*args, None)
    return L.cgrt_winding_numbers_brute(*args) if form == "brute" else L.cgrt_winding_numbers(*args)


BAD_BETA = (0.5, float("nan"), -1.0, -INF, 0.999)


@pytest.mark.parametrize("form", ["host", "device", "work", "brute"])
def test_argument_checks_of_the_list_entries_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    dev, work, brute = form == "device", form == "work", form == "brute"
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(params=None) == E_NO_DEVICE, "NULL params: all defaults"
    assert c(n=0x7FFFFFFF) == E_NO_DEVICE
    for beta in (0.0, 1.0, 2.0, 1e30, INF):
        assert c(params=_params(pkg, beta)) == E_NO_DEVICE, beta
    assert c(params=_params(pkg, 2.0, float("nan"))) == E_NO_DEVICE and c(params=_params(pkg, 2.0, -1.0)) == E_NO_DEVICE, "any threshold"
    if not work:
        assert c(w=None) == E_NO_DEVICE and c(inside=None) == E_NO_DEVICE, "either output may be NULL"
    # 1 - 4
    assert c(handle=None) == E_ARG and "scene" in _err(pkg)
    assert c(points=None) == E_ARG and "NULL" in _err(pkg)
    assert c(w=None, inside=None) == E_ARG and "neither" in _err(pkg)
    assert c(points=None, n=0) == E_NO_DEVICE, "NULL points with n == 0 are allowed"
    assert c(n=0x80000000) == E_ARG and "0x7fffffff" in _err(pkg)
    # 5: beta (the brute entry does not read it)
    for beta in BAD_BETA:
        assert c(params=_params(pkg, beta)) == (E_NO_DEVICE if brute else E_ARG), beta
        assert brute or "beta" in _err(pkg)
    # 6 (device form): d_points and d_w 4-byte aligned; d_inside is bytes
    for kw in ({"points": 2}, {"w": 2}):
        if work and "w" in kw:
            continue
        assert c(**kw) == (E_ARG if dev else E_NO_DEVICE), kw
        assert not dev or "aligned" in _err(pkg)
    if not work:
        assert c(inside=1) == E_NO_DEVICE
    # the order
    bad = _params(pkg, 0.5)
    assert c(handle=None, points=None, w=None, inside=None, n=1 << 40, params=bad) == E_ARG and "scene" in _err(pkg)
    assert c(points=None, w=None, inside=None, n=1 << 40, params=bad) == E_ARG and "NULL" in _err(pkg) and "neither" not in _err(pkg)
    assert c(w=None, inside=None, n=1 << 40, params=bad) == E_ARG and "neither" in _err(pkg)
    assert c(points=2, n=1 << 40, params=bad) == E_ARG and "0x7fffffff" in _err(pkg)
    if not brute:
        assert c(points=2, params=bad) == E_ARG and "beta" in _err(pkg)
    assert c(points=2) == (E_ARG if dev else E_NO_DEVICE)


@pytest.mark.parametrize("form", ["grid", "grid_device"])
def test_argument_checks_of_the_grid_entries_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    dev = form == "grid_device"
    assert c() == E_NO_DEVICE and c(params=None) == E_NO_DEVICE
    assert c(w=None) == E_NO_DEVICE and c(inside=None) == E_NO_DEVICE
    assert c(grid=_grid(pkg, (1 << 24, 1, 127))) == E_NO_DEVICE
    assert c(grid=_grid(pkg, spacing=(0.0, -1.0, 1e30))) == E_NO_DEVICE, "zero or negative spacing is allowed"
    assert c(handle=None) == E_ARG and "scene" in _err(pkg)
    assert c(grid=None) == E_ARG and "grid" in _err(pkg)
    assert c(w=None, inside=None) == E_ARG and "neither" in _err(pkg)
    for dims in ((0, 1, 1), (1, 1, 0), ((1 << 24) + 1, 1, 1)):
        assert c(grid=_grid(pkg, dims)) == E_ARG and "2^24" in _err(pkg), dims
    for dims in ((1 << 24, 128, 1), (2048, 1024, 1024)):
        assert c(grid=_grid(pkg, dims)) == E_ARG and "0x7fffffff" in _err(pkg), dims
    assert c(grid=_grid(pkg, origin=(0, float("nan"), 0))) == E_ARG and "finite" in _err(pkg)
    for beta in BAD_BETA:
        assert c(params=_params(pkg, beta)) == E_ARG and "beta" in _err(pkg), beta
    assert c(w=2) == (E_ARG if dev else E_NO_DEVICE)
    assert not dev or "aligned" in _err(pkg)
    # the order
    bad, big = _params(pkg, 0.5), _grid(pkg, (1 << 24, 1 << 24, 2))
    assert c(handle=None, grid=None, w=None, inside=None, params=bad) == E_ARG and "scene" in _err(pkg)
    assert c(grid=None, w=None, inside=None, params=bad) == E_ARG and "grid" in _err(pkg)
    assert c(grid=big, w=None, inside=None, params=bad) == E_ARG and "neither" in _err(pkg)
    assert c(grid=big, w=2, params=bad) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(w=2, params=bad) == E_ARG and "beta" in _err(pkg)


def test_numpy_forms_on_a_host_only_scene(pkg, host_scene):
    pts = np.zeros((4, 3), np.float32)
    for f in (host_scene.winding_numbers, host_scene.winding_numbers_brute, host_scene.debug_winding_work,
              lambda p: host_scene.winding_numbers(p, want="inside"), lambda p: host_scene.winding_grid((0, 0, 0), (1, 1, 1), (2, 2, 2))):
        with pytest.raises(pkg.CgrtError) as e:
            f(pts)
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        host_scene.winding_numbers(np.zeros((4, 2), np.float32))  # (not n x 3)
    with pytest.raises(ValueError):
        host_scene.winding_numbers(pts, want=("sdf",))
    with pytest.raises(pkg.CgrtError) as e:
        host_scene.winding_numbers(pts, beta=0.5)
    assert e.value.code == E_ARG


# ---- the cluster tree, read from host-only scenes ----
_trees = {}


def _tree(pkg, scene_data, name):
    """(scene data, the tree as the library built it, the records in record order), once per scene."""
    if name not in _trees:
        sd = _scene(pkg, scene_data, name)
        sc = pkg.Scene(sd, device=-1)
        h0 = sc.layout_hash() if hasattr(sc, "layout_hash") else None
        tree = sc.debug_winding_tree()
        again = sc.debug_winding_tree()
        assert all(np.array_equal(tree[k].view(np.uint8), again[k].view(np.uint8)) for k in tree), "one tree per scene"
        assert h0 is None or sc.layout_hash() == h0, "the existing arrays are untouched"
        sc.close()
        _trees[name] = (sd, tree, wr.records(sd, tree))
    return _trees[name]


def _dist2_f32(v, c):
    """((dx * dx + dy * dy) + dz * dz) in float32, d = v - c."""
    with np.errstate(all="ignore"):
        d = v.astype(np.float32) - c.astype(np.float32)
        out = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("name", ["cube", "blob", "dodge", "dragon"] + [f"blob:{k}" for k in TRUNCATIONS])
def test_tree_invariants(pkg, scene_data, name):
    sd, tree, recs = _tree(pkg, scene_data, name)
    T = len(recs)
    assert T == int(np.asarray(sd.tri).size // 3) and sorted(tree["record_prims"].tolist()) == list(range(T)), "every triangle is one record"
    cl, off = tree["clusters"], tree["level_offsets"]
    counts, prev = [], T
    while True:
        prev = -(-prev // 8)
        counts.append(prev)
        if prev <= 8:
            break
    assert list(np.diff(off)) == counts and off[0] == 0 and len(cl) == sum(counts) and len(counts) <= 9, (list(off), counts)
    assert (cl[:, 7] == 0).all()
    ref = wr.clusters(recs)
    assert [len(lv["c"]) for lv in ref] == counts
    eps = 2.0 ** -24
    for L, lv in enumerate(ref):
        C = cl[off[L] : off[L + 1]]
        for i in range(len(C)):
            v = recs[lv["first"][i] : lv["last"][i]].reshape(-1, 3)
            q = _dist2_f32(v, C[i, 0:3])
            assert (q <= C[i, 3]).all(), (name, L, i, float(q.max()), float(C[i, 3]))
            assert q.max() == C[i, 3], "the radius is tight: the largest of them"
        bound = 8 * eps * lv["abs"][:, None]
        assert (np.abs(C[:, 4:7].astype(np.float64) - lv["n"]) <= bound).all(), (name, L)
        if L > 0:
            kids = cl[off[L - 1] : off[L], 4:7].astype(np.float64)
            sums = np.add.reduceat(kids, np.arange(0, len(kids), 8), axis=0)
            assert (np.abs(C[:, 4:7].astype(np.float64) - sums) <= bound).all(), (name, L, "children")
        # the centre: the area-weighted mean of the centroids, rounded once (one f32 rounding of a float64 value, some slack for the sums)
        scale = np.abs(recs).max()
        assert (np.abs(C[:, 0:3].astype(np.float64) - lv["c"]) <= 4 * eps * scale).all(), (name, L, "centre")


# ---- accuracy of the tree form against the float64 sum over every triangle ----
BETAS = (2.0, 3.0, 4.0, INF)
NPTS, SEED = 385, 11
BAND = 0.05


@pytest.mark.parametrize("name", ["cube", "blob", "monkey", "dragon", "dodge"])
def test_tree_form_against_the_float64_winding_number(pkg, scene_data, name):
    sd, tree, recs = _tree(pkg, scene_data, name)
    pts = sr.sign_queries(sd, NPTS, SEED)
    assert len(pts) == NPTS
    w64 = sr.winding64(sd, pts)
    keep = np.abs(np.abs(w64) - 0.5) >= BAND
    truth = np.abs(w64) > 0.5
    print(f"\n{name} ({len(recs)} triangles, {NPTS} points, {100.0 * (~keep).mean():.2f} % in the band, {100.0 * truth.mean():.1f} % inside)")
    print("   beta   max error  mean error  clusters/pt  dipoles/pt  triangles/pt  verdicts differing outside the band")
    worst = {}
    for beta in BETAS:
        w, work = wr.walk(tree, recs, pts, beta, np.float64)
        err = np.abs(w - w64)
        worst[beta] = float(err.max())
        wrong = int(((np.abs(w) > 0.5) != truth)[keep].sum())
        print(f"  {beta:5.1f}  {err.max():.2e}   {err.mean():.2e}   {work[0] / NPTS:9.1f}  {work[1] / NPTS:9.1f}  {work[2] / NPTS:11.1f}   {wrong}")
        if beta == INF:
            assert work[1] == 0 and work[2] == NPTS * len(recs), "no cluster is far: every triangle of every point"
            assert err.max() <= 1e-12, "the same sum"
        if beta == 2.0:
            assert wrong == 0, (name, wrong)
    assert (~keep).sum() <= 0.02 * NPTS
    noise = 1e-12  # (float64 sums of a few thousand terms: where every beta is exact the three errors are rounding noise)
    assert worst[3.0] <= worst[2.0] + noise and worst[4.0] <= worst[3.0] + noise, worst
    assert truth.any() and (~truth).any()


@pytest.mark.parametrize("name", ["cube", "dragon"])
def test_verdict_is_the_parity_vote_on_closed_meshes(pkg, orc, scene_data, name):
    sd, tree, recs = _tree(pkg, scene_data, name)
    assert sr.is_closed(sd)
    pts = sr.sign_queries(sd, NPTS, SEED)
    keep = cr.dist64(sd, pts).min(axis=1) > 1e-4 * sr.extent(sd)
    _, inside = sdf_ref.reference(orc, sd, pts, pkg.INSIDE_DIRECTIONS)
    w, _ = wr.walk(tree, recs, pts, 2.0, np.float64)
    assert (~keep).sum() <= 0.02 * NPTS and inside[keep].any() and (~inside[keep]).any()
    bad = np.flatnonzero(keep & ((np.abs(w) > 0.5) != inside))
    assert len(bad) == 0, (name, len(bad), pts[bad[0]], float(w[bad[0]]))

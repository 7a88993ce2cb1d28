"""No GPU: closest-point queries (cgrt_closest_points*; include/cgrt.h).

* tests/closest_ref.py -- the numpy float32 restatement of the definition the GPU tests hold the device to, bit for bit -- against a float64
  referee (the same region walk in float64, without the clamp).  For EVERY query, none classed or skipped,

      |sqrt(dist2_32) - D64|                  <= K * 2^-24 * scale
      d64(p, returned triangle) - D64         <= K * 2^-24 * scale

  with D64 the float64 minimum over all triangles and scale = max(1, |p|inf, largest |coordinate| of the scene).  K is twice the largest
  ratio measured on these very inputs on the CPU (`_inputs`: the five finite query families of closest_ref, 300 of each per scene, 80 on
  dodge).  Largest ratios of the first / second quantity: triangle 1.41 / 0, cube 1.80 / 0, cornell 2.83 / 0.55, monkey 1.36 / 0.27,
  blob 1.68 / 0.46, dodge 2.19 / 0.12.
* The lemma the tree search rests on: the box lower bound lb2 never exceeds dist2, in float32 with no slack, for each triangle's own box
  and for randomly grown boxes.
* Its premise: on host-only scenes every box of cgrt_get_nodes contains the vertices of the triangles cgrt_leaf_prims lists under it.
* The entries are exported and check their arguments in the documented order on a host-only scene."""
import ctypes as C

import numpy as np
import pytest

import closest_ref as cr

E_ARG, E_NO_DEVICE = -1, -2
ENTRIES = ("cgrt_closest_points", "cgrt_closest_points_device", "cgrt_closest_points_brute", "cgrt_debug_closest_work")
SCENES = ("triangle", "cube", "cornell", "monkey", "blob", "dodge")
K = 2 * 2.83  # twice the largest ratio measured over `_inputs` of the six scenes (module docstring)
FAMILIES = (cr.uniform_queries, cr.surface_queries, cr.vertex_queries, cr.edge_queries, cr.far_queries)

_cache = {}


def _inputs(scene_data, name):
    """The five finite query families (seeds 31..35), their float32 results and the float64 distances to every triangle."""
    if name not in _cache:
        sd = scene_data(name)
        m = 80 if name == "dodge" else 300
        q = np.concatenate([f(sd, m, 31 + i) for i, f in enumerate(FAMILIES)])
        _cache[name] = (sd, q, cr.brute(sd, q), cr.dist64(sd, q))
    return _cache[name]


@pytest.mark.parametrize("name", SCENES)
def test_restatement_against_float64(scene_data, name):
    sd, q, r, D = _inputs(scene_data, name)
    assert (r["prim_id"] != cr.NO_PRIM).all(), "unbounded queries always find a triangle"
    D64 = D.min(axis=1)
    scale = np.maximum(1.0, np.maximum(np.abs(q.astype(np.float64)).max(axis=1), cr.scene_scale(sd)))
    unit = 2.0 ** -24 * scale
    r1 = np.abs(np.sqrt(r["dist2"].astype(np.float64)) - D64) / unit
    r2 = (D[np.arange(len(q)), r["prim_id"]] - D64) / unit
    print(f"{name}: {len(q)} queries x {sd.ntris} triangles, largest ratios {r1.max():.3f} (distance) {r2.max():.3f} (returned triangle), K {K}")
    assert r1.max() <= K, (name, float(r1.max()), int(r1.argmax()))
    assert r2.max() <= K, (name, float(r2.max()), int(r2.argmax()))
    # the record is consistent: the point is the barycentric mix up to rounding, the weights sum to 1 up to rounding
    a, b, c = cr.tri_verts(sd, np.float64)
    k, w = r["prim_id"], r["bary"].astype(np.float64)
    mix = a[k] * w[:, 0:1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:3]
    assert np.abs(w.sum(axis=1) - 1).max() < 1e-5
    assert (np.abs(mix - r["point"]).max(axis=1) <= 64 * unit).all()


@pytest.mark.parametrize("name", SCENES)
def test_box_lower_bound_never_exceeds_dist2(scene_data, name):
    sd, q, _, _ = _inputs(scene_data, name)
    q = np.concatenate([q, cr.mixed_queries(sd, 64, 5)])  # (with the NaN and the inf point: a NaN never compares greater)
    a, b, c = cr.tri_verts(sd)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    rng = np.random.default_rng(17)
    ext = (hi - lo).max()
    step = max(1, (1 << 18) // len(a))
    triples = 0
    for s in range(0, len(q), step):
        p = q[s : s + step, None, :]
        _, d2, _, _, _ = cr.closest_tri32(p, a, b, c)
        assert not (cr.box_lb2(lo, hi, p) > d2).any(), (name, "own box")
        for _ in range(3):  # boxes that contain the triangle's: each side pushed out by a random amount, a third of them not at all
            g = rng.random((2,) + lo.shape).astype(np.float32) * np.float32(ext) * (rng.random((2,) + lo.shape) < 0.67)
            glo, ghi = (lo - g[0]).astype(np.float32), (hi + g[1]).astype(np.float32)
            assert (glo <= lo).all() and (ghi >= hi).all()
            assert not (cr.box_lb2(glo, ghi, p) > d2).any(), (name, "grown box")
        triples += 4 * d2.size
    assert triples >= 4 * len(a)


@pytest.mark.parametrize("name", SCENES)
def test_every_node_box_contains_its_triangles(pkg, scene_data, name):
    sd = scene_data(name)
    sc = pkg.Scene(sd, device=-1)
    try:
        meta, boxes = sc.nodes()
        assert len(meta) >= 1
        a, b, c = cr.tri_verts(sd)
        seen = 0
        for node in range(len(meta)):
            prims = sc.leaf_prims(node)
            assert len(prims) == meta[node, 4] and len(prims) >= 1
            v = np.concatenate([a[prims], b[prims], c[prims]])
            lo, hi = boxes[node, 0:3], boxes[node, 3:6]
            assert (v >= lo).all() and (v <= hi).all(), (name, node)
            assert (v.min(axis=0) == lo).all() and (v.max(axis=0) == hi).all(), (name, node, "the exact min / max")
            seen += int(meta[node, 0] != 0) * len(prims)
        assert seen == sd.ntris, "every triangle under exactly one leaf"
    finally:
        sc.close()


def test_entries_are_exported(pkg):
    L = C.CDLL(pkg.LIB_PATH)
    for sym in ENTRIES:
        assert sym in pkg.EXPORTS and hasattr(L, sym), sym
    for name in ("closest_points", "closest_points_brute", "closest_points_device", "closest_points_tensor", "debug_closest_work"):
        assert callable(getattr(pkg.Scene, name, None)), name
    assert pkg.CLOSEST_DTYPE == cr.CLOSEST_DTYPE and pkg.CLOSEST_DTYPE.itemsize == 32


@pytest.fixture(scope="module")
def host_scene(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=-1)
    yield s
    s.close()


_POINTS = np.zeros(16 * 3 + 4, np.float32)
_OUT = np.zeros(16 * 8 + 4, np.float32)


def _err(pkg):
    return pkg.lib().cgrt_last_error().decode()


def _call(pkg, sc, form, handle="ok", points=0, n=16, max_dist2=np.inf, out=0):
    """points / out: a byte offset into the module's arrays, or None for NULL."""
    p = lambda a, off: None if off is None else C.c_void_p(a.ctypes.data + off)  # noqa: E731
    L = pkg.lib()
    f = {"host": L.cgrt_closest_points, "brute": L.cgrt_closest_points_brute, "device": L.cgrt_closest_points_device,
         "work": L.cgrt_debug_closest_work}[form]
    args = [sc._h if handle == "ok" else None, p(_POINTS, points), n, float(max_dist2), p(_OUT, out)]
    return f(*args, None) if form == "device" else f(*args)


@pytest.mark.parametrize("form", ["host", "brute", "device", "work"])
def test_argument_checks_and_their_order(pkg, host_scene, form):
    c = lambda **kw: _call(pkg, host_scene, form, **kw)  # noqa: E731
    assert c() == E_NO_DEVICE, "an otherwise valid call on a host-only scene"
    assert c(n=0x7fffffff) == E_NO_DEVICE and c(max_dist2=0.0) == E_NO_DEVICE and c(max_dist2=1.5) == E_NO_DEVICE
    # rule 1: NULL scene
    assert c(handle=None) == E_ARG and "scene" in _err(pkg)
    # rule 2: NULL points or out with n > 0
    assert c(points=None) == E_ARG and "NULL" in _err(pkg)
    assert c(out=None) == E_ARG and "NULL" in _err(pkg)
    assert c(points=None, out=None, n=0) == E_NO_DEVICE, "NULL arrays with n == 0 are allowed"
    # rule 3: n > 0x7fffffff
    assert c(n=0x80000000) == E_ARG and "0x7fffffff" in _err(pkg)
    # rule 4: max_dist2 NaN or negative
    assert c(max_dist2=np.nan) == E_ARG and "max_dist2" in _err(pkg)
    assert c(max_dist2=-1.0) == E_ARG and "max_dist2" in _err(pkg)
    assert c(max_dist2=-np.inf) == E_ARG and "max_dist2" in _err(pkg)
    # rule 5 (device form): every pointer 4-byte aligned
    for kw in ({"points": 2}, {"out": 2}):
        assert c(**kw) == (E_ARG if form == "device" else E_NO_DEVICE), kw
        assert form != "device" or "aligned" in _err(pkg)
    # the order
    assert c(handle=None, points=None, n=1 << 40, max_dist2=np.nan, out=2) == E_ARG and "scene" in _err(pkg)
    assert c(points=None, n=1 << 40, max_dist2=np.nan, out=2) == E_ARG and "NULL" in _err(pkg)
    assert c(n=1 << 40, max_dist2=np.nan, out=2) == E_ARG and "0x7fffffff" in _err(pkg)
    assert c(max_dist2=np.nan, out=2) == E_ARG and "max_dist2" in _err(pkg)
    assert c(out=2) == (E_ARG if form == "device" else E_NO_DEVICE)


def test_numpy_forms_on_a_host_only_scene(pkg, host_scene):
    for f in (host_scene.closest_points, host_scene.closest_points_brute, host_scene.debug_closest_work):
        with pytest.raises(pkg.CgrtError) as e:
            f(np.zeros((4, 3), np.float32))
        assert e.value.code == E_NO_DEVICE
    with pytest.raises(ValueError):
        host_scene.closest_points(np.zeros((4, 2), np.float32))  # (not n x 3)

"""GPU tests of the closest-point queries (include/cgrt.h cgrt_closest_points*; Scene.closest_points and its _brute / _device / _tensor
forms, debug_closest_work).

Everything is compared as bytes (conftest.same_bits on the floats, equality on the ids): the device's tree search (k_closest), the
device's brute force (k_closest_brute) and tests/closest_ref.py -- the numpy restatement of the definition that tests/test_closest_cpu.py
holds to a float64 referee -- give the same records.  The query lists interleave the families of closest_ref (uniform in the grown scene
box, on random triangles, exact vertices -- ties go to the lowest prim_id --, edge midpoints, far points) and carry one NaN and one inf
point.  Every device output lies between guards of sentinel bytes."""
import dataclasses
import threading

import numpy as np
import pytest

import closest_ref as cr
from conftest import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
INF = float("inf")
LENGTHS = (1, 63, 64, 65, 4097)
NMAX = max(LENGTHS)


class Guarded:
    """nbytes of device memory between two guards, all of it sentinel bytes before the call."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def tensor(self, shape):
        return self.buf[PAD : PAD + self.n].view(torch.float32).view(tuple(shape))

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n :] == SENTINEL).all())


def _same(a, b):
    """Two CLOSEST_DTYPE arrays, field by field."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ids = bool((a["prim_id"] == b["prim_id"]).all())
    return ids and all(bool(same_bits(a[f], b[f]).all()) for f in ("point", "dist2", "bary"))


def _first_difference(a, b):
    for i in range(len(a)):
        if not _same(a[i : i + 1], b[i : i + 1]):
            return i, a[i], b[i]
    return None


def _records(pkg, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(pkg.CLOSEST_DTYPE).reshape(-1)


_scenes = {}
_refs = {}


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    """name -> (SceneData, Scene on device 0), created once."""

    def get(name):
        if name not in _scenes:
            sd = scene_data(name)
            _scenes[name] = (sd, pkg.Scene(sd, device=0))
        return _scenes[name]

    yield get
    for _, sc in _scenes.values():
        sc.close()
    _scenes.clear()


def _queries(sd, name):
    """The scene's one query list (NMAX mixed queries) and, computed once, the restatement's records for a prefix of it."""
    if name not in _refs:
        _refs[name] = [cr.mixed_queries(sd, NMAX, 11), None, 0]
    return _refs[name][0]


def _reference(sd, name, n):
    q = _queries(sd, name)
    e = _refs[name]
    if e[1] is None or e[2] < n:
        e[1], e[2] = cr.brute(sd, q[:n]), n
    return e[1][:n]


# ---- 1. parity: tree == brute == restatement ----
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["triangle", "cube", "cornell", "monkey", "blob"])
def test_tree_brute_and_restatement_agree(pkg, scenes, name, n):
    sd, sc = scenes(name)
    q = _queries(sd, name)[:n]
    ref = _reference(sd, name, NMAX)[:n]
    tree, brute = sc.closest_points(q), sc.closest_points_brute(q)
    assert tree.dtype == pkg.CLOSEST_DTYPE and len(tree) == n
    assert _same(brute, ref), (name, n, "brute force against the restatement", _first_difference(brute, ref))
    assert _same(tree, brute), (name, n, "tree search against brute force", _first_difference(tree, brute))
    finite = np.isfinite(q).all(axis=1)
    assert (tree["prim_id"][finite] < sd.ntris).all(), "an unbounded finite query always finds a triangle"
    miss = tree[~finite]
    assert (miss["prim_id"] == cr.NO_PRIM).all() and np.isinf(miss["dist2"]).all() and not miss["point"].any() and not miss["bary"].any()
    if n >= 63:
        assert (~finite).sum() == 2, "the NaN and the inf point"
        at_vertex = tree[2::5]  # (family 2: exact vertex positions)
        assert (at_vertex["dist2"][np.isfinite(q[2::5]).all(axis=1)] == 0).all()
        if sd.ntris > 1:
            a, b, c = cr.tri_verts(sd)
            lowest = np.array([np.flatnonzero(((a == p).all(1)) | ((b == p).all(1)) | ((c == p).all(1)))[0] for p in q[2::5][:12]])
            assert (at_vertex["prim_id"][:12] <= lowest).all(), "ties go to the lowest prim_id (of the triangles that share the vertex, at least)"


def test_dodge_tree_equals_brute_and_brute_the_restatement(pkg, scenes):
    sd, sc = scenes("dodge")
    assert sc.num_subnodes() > 0, "the scene with in-leaf accelerators"
    q = _queries(sd, "dodge")
    tree, brute = sc.closest_points(q), sc.closest_points_brute(q)
    assert _same(tree, brute), _first_difference(tree, brute)
    ref = _reference(sd, "dodge", 256)
    assert _same(brute[:256], ref), _first_difference(brute[:256], ref)


# ---- 2. the radius ----
@pytest.mark.parametrize("name", ["cornell", "blob", "dodge"])
def test_radius(pkg, scenes, name):
    sd, sc = scenes(name)
    n = 128 if name == "dodge" else 1024
    vq = cr.vertex_queries(sd, n, 41)
    at0 = sc.closest_points(vq, 0.0)
    assert (at0["prim_id"] < sd.ntris).all() and (at0["dist2"] == 0).all(), "max_dist2 = 0 still accepts dist2 == 0"
    assert _same(at0, sc.closest_points_brute(vq, 0.0)) and _same(at0, cr.brute(sd, vq, 0.0))
    uq = cr.uniform_queries(sd, n, 42)
    unbounded = sc.closest_points(uq, INF)
    assert (unbounded["prim_id"] < sd.ntris).all()
    r2 = float(np.median(unbounded["dist2"]))
    got = sc.closest_points(uq, r2)
    hit = got["prim_id"] != cr.NO_PRIM
    assert hit.any() and (~hit).any(), (name, "a mix of hits and misses", int(hit.sum()))
    assert (got["dist2"][hit] <= np.float32(r2)).all() and np.isinf(got["dist2"][~hit]).all()
    assert _same(got[hit], unbounded[hit]), "a query inside the radius gets its unbounded answer"
    assert (unbounded["dist2"][~hit] > np.float32(r2)).all()
    assert _same(got, sc.closest_points_brute(uq, r2)) and _same(got, cr.brute(sd, uq, r2))
    assert _same(unbounded, sc.closest_points_brute(uq, INF))


# ---- 3. configurations ----
def test_linear_leaves(pkg, scenes):
    sd, accel = scenes("dodge")
    q = _queries(sd, "dodge")
    try:
        pkg.set_leaf_accel(False)
        sc = pkg.Scene(sd, device=0)
    finally:
        pkg.set_leaf_accel(True)
    try:
        got = sc.closest_points(q)
        want = accel.closest_points_brute(q)
        assert _same(got, want), _first_difference(got, want)
    finally:
        sc.close()


def test_long_runs_and_deep_accelerators(pkg):
    """Leaves of ~34 triangles: under the default two triangles per run their accelerators are three levels deep; under 32 per run the
    runs hold 17 and more records (a run reference with bit 30 set)."""
    sd = pkg.scenes.make_blob(70000, seed=3)
    q = cr.mixed_queries(sd, 1024, 13)
    want = None
    for run in (0, 32):
        try:
            pkg.set_leaf_accel(True, run)
            sc = pkg.Scene(sd, device=0)
        finally:
            pkg.set_leaf_accel(True)
        try:
            assert sc.num_subnodes() > 0
            if want is None:
                want = sc.closest_points_brute(q)
            got = sc.closest_points(q)
            assert _same(got, want), (run, _first_difference(got, want))
        finally:
            sc.close()


def test_spheres_beside_the_mesh_are_ignored(pkg, scenes):
    sd, plain = scenes("blob")
    hi = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3].max(0)
    sph = np.asarray([[hi[0], hi[1], 0.0, 0.45 * hi[0], -1], [-hi[0], 0.0, hi[2], 0.4 * hi[0], 0]], np.float32)
    sc = pkg.Scene(dataclasses.replace(sd, spheres=sph, name="blob+spheres"), device=0)
    try:
        q = _queries(sd, "blob")
        got = sc.closest_points(q)
        assert _same(got, plain.closest_points(q)) and _same(got, sc.closest_points_brute(q))
    finally:
        sc.close()


def test_a_scene_without_meshes_misses_everything(pkg, scene_data):
    sd = scene_data("spheres")
    assert sd.ntris == 0 and len(sd.spheres) > 0
    sc = pkg.Scene(sd, device=0)
    try:
        q = np.random.default_rng(3).normal(size=(130, 3)).astype(np.float32)
        for got in (sc.closest_points(q), sc.closest_points_brute(q), sc.closest_points(q, 4.0)):
            assert _same(got, cr.miss_records(len(q)))
        assert sc.debug_closest_work(q) == (0, 0)
    finally:
        sc.close()


def test_nan_and_inf_vertices(pkg, scenes):
    clean, _ = scenes("blob")
    pos = np.asarray(clean.pos_nrm, np.float32).reshape(-1, 6).copy()
    tri = np.asarray(clean.tri).reshape(-1, 3)
    pos[tri[100, 1], 0] = np.nan
    pos[tri[900, 2], 1] = np.inf
    sd = dataclasses.replace(clean, pos_nrm=pos, name="blob+nan+inf")
    q = _queries(clean, "blob")[:1024]
    sc = pkg.Scene(sd, device=0)
    try:
        tree, brute, ref = sc.closest_points(q), sc.closest_points_brute(q), cr.brute(sd, q)
        assert _same(brute, ref), _first_difference(brute, ref)
        assert _same(tree, brute), _first_difference(tree, brute)
        assert (tree["prim_id"] != 100).all(), "a triangle with a NaN coordinate never qualifies"
    finally:
        sc.close()


# ---- 4. the device form ----
@pytest.mark.parametrize("n", LENGTHS)
def test_device_form_between_guards_on_a_side_stream(pkg, scenes, n):
    sd, sc = scenes("blob")
    q = _queries(sd, "blob")[:n]
    ref = _reference(sd, "blob", NMAX)[:n]
    d_q = torch.from_numpy(q.copy()).cuda()
    g = Guarded(32 * n)
    out = g.tensor((n, 8))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    res = sc.closest_points_tensor(d_q, out=out, stream=side)
    side.synchronize()
    assert res["out"] is out, "out= is returned as passed"
    assert g.intact()
    got = _records(pkg, out)
    assert _same(got, ref), (n, _first_difference(got, ref))
    assert res["point"].shape == (n, 3) and res["dist2"].shape == (n,) and res["bary"].shape == (n, 3)
    assert res["prim_id"].dtype == torch.int32 and (res["prim_id"].cpu().numpy().view(np.uint32) == ref["prim_id"]).all()
    assert same_bits(res["dist2"].cpu().numpy(), ref["dist2"]).all() and same_bits(res["bary"].cpu().numpy(), ref["bary"]).all()
    # a new tensor on the current stream, with a radius
    r2 = float(np.median(ref["dist2"][np.isfinite(ref["dist2"])]))
    res = sc.closest_points_tensor(d_q, max_dist2=r2)
    assert _same(_records(pkg, res["out"]), sc.closest_points_brute(q, r2))
    with pytest.raises(ValueError):
        sc.closest_points_tensor(d_q, out=torch.zeros((n, 7), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        sc.closest_points_tensor(d_q.cpu())


def test_device_form_checks_its_buffers(pkg, scenes):
    sd, sc = scenes("cube")
    d_q = torch.zeros((16, 3), dtype=torch.float32, device="cuda")
    d_o = torch.zeros((16, 8), dtype=torch.float32, device="cuda")
    host = np.zeros((16, 8), np.float32)
    sc.closest_points_device(d_q.data_ptr(), 16, d_o.data_ptr())
    torch.cuda.synchronize()
    with pytest.raises(pkg.CgrtError) as e:
        sc.closest_points_device(d_q.data_ptr(), 16, host.ctypes.data)
    assert e.value.code == -1
    with pytest.raises(pkg.CgrtError) as e:
        sc.closest_points_device(d_q.data_ptr(), 16, d_o.data_ptr(), max_dist2=float("nan"))
    assert e.value.code == -1
    sc.closest_points_device(0, 0, 0)  # n == 0 touches nothing


def test_four_threads_on_one_scene(pkg, scenes):
    sd, sc = scenes("blob")
    q = _queries(sd, "blob")
    single = sc.closest_points(q).tobytes()
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                results[k] = sc.closest_points(q).tobytes()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(r == single for r in results), "the host form is concurrent on one scene"


# ---- 5. the cull fires ----
def test_work_on_dodge(pkg, scenes):
    sd, sc = scenes("dodge")
    q = cr.surface_queries(sd, 4096, 51)
    nodes, tris = sc.debug_closest_work(q)
    mean_tris, mean_nodes = tris / len(q), nodes / len(q)
    print(f"dodge, {len(q)} on-surface queries: {mean_nodes:.1f} node steps and {mean_tris:.1f} triangles evaluated per query of {sd.ntris}")
    assert nodes > 0 and tris >= len(q)
    assert mean_tris < sd.ntris / 2, mean_tris

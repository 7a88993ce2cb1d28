"""GPU tests of the neighbour queries (include/cgrt.h cgrt_count_neighbors*, cgrt_list_neighbors*; Scene.count_neighbors,
list_neighbors, nearest_triangles, list_neighbors_brute, debug_neighbor_work and the _device / _tensor forms).

Everything is compared as bytes: the device's tree search (k_neighbors), the device's brute force (k_neighbors<.., BRUTE>) and
tests/neighbors_ref.py -- the numpy restatement that tests/test_neighbors_cpu.py holds to a float64 referee -- give the same counts
and the same records.  The query lists are closest_ref.mixed_queries (uniform, on the surface, exact vertices -- ties at dist2 == 0 --,
edge midpoints, far points, one NaN and one inf point).  Every device output of the _tensor tests lies between guards of sentinel bytes."""
import dataclasses
import threading

import numpy as np
import pytest

import closest_ref as cr
import neighbors_ref as nr
from conftest import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
INF = float("inf")
LENGTHS = (1, 63, 64, 65, 4097)
NMAX = max(LENGTHS)
KS = (1, 3, 8)
SCENES = ("triangle", "cube", "cornell", "monkey", "blob")


class Guarded:
    """nbytes of device memory between two guards, all of it sentinel bytes before the call."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def tensor(self, shape, dtype=torch.float32):
        return self.buf[PAD : PAD + self.n].view(dtype).view(tuple(shape))

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n :] == SENTINEL).all())


def _records(t):
    torch.cuda.synchronize()
    return np.ascontiguousarray(t.cpu().numpy()).view(nr.NEIGHBOR_DTYPE).reshape(t.shape[:-1])


_scenes = {}
_queries = {}
_full = {}


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


def _q(sd, name):
    if name not in _queries:
        _queries[name] = cr.mixed_queries(sd, NMAX, 11)
    return _queries[name]


def _r2(sd, frac):
    return float(np.float32(np.float32(frac * nr.extent(sd)) ** 2))


def _reference(sd, name, frac):
    """The restatement's full answer for the scene's NMAX queries at the radius frac * extent (None: unbounded), computed once; a
    prefix of the queries has a prefix of it."""
    if (name, frac) not in _full:
        _full[(name, frac)] = nr.neighbors(sd, _q(sd, name), None, INF if frac is None else _r2(sd, frac))
    return _full[(name, frac)]


def _prefix(full, n):
    off, rec = full
    return off[: n + 1], rec[: off[n]]


# ---- 1. parity: tree == brute == restatement ----
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name,frac", [(s, 0.05) for s in SCENES] + [("monkey", 0.1)])
def test_tree_brute_and_restatement_agree(pkg, scenes, name, frac, n):
    sd, sc = scenes(name)
    q, r2 = _q(sd, name)[:n], _r2(sd, frac)
    ref = _prefix(_reference(sd, name, frac), n)
    want_counts = np.diff(ref[0]).astype(np.uint32)
    counts = sc.count_neighbors(q, max_dist2=r2)
    assert counts.dtype == np.uint32 and (counts == want_counts).all(), (name, n, "counts", np.flatnonzero(counts != want_counts)[:4])
    off, rec = sc.list_neighbors(q, max_dist2=r2)
    boff, brec = sc.list_neighbors_brute(q, max_dist2=r2)
    assert rec.dtype == pkg.NEIGHBOR_DTYPE and (boff == ref[0]).all() and (off == ref[0]).all()
    assert nr.same(brec, ref[1]), (name, n, "brute force against the restatement", nr.first_difference(brec, ref[1]))
    assert nr.same(rec, brec), (name, n, "tree search against brute force", nr.first_difference(rec, brec))
    for k in KS:
        want = nr.nearest(ref, k)
        tree = sc.nearest_triangles(q, k, max_dist2=r2)
        brute, bc = sc.list_neighbors_brute(q, max_dist2=r2, k=k)
        assert nr.same(brute, want), (name, n, k, "brute force against the restatement", nr.first_difference(brute, want))
        assert nr.same(tree, brute), (name, n, k, "tree search against brute force", nr.first_difference(tree, brute))
        assert (bc == want_counts).all()
    if n == NMAX and name != "triangle":
        assert counts.max() >= 3 and (counts == 0).any(), "lists of several neighbours, and queries with none"


# ---- 2. N1: k = 1 is closest_points ----
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_k1_is_closest_points(pkg, scenes, name, bounded):
    sd, sc = scenes(name)
    q = _q(sd, name)
    r2 = _r2(sd, 0.05) if bounded else INF
    near = sc.nearest_triangles(q, 1, max_dist2=r2)[:, 0]
    cp = sc.closest_points(q, r2)
    assert (near["prim_id"] == cp["prim_id"]).all() and same_bits(near["dist2"], cp["dist2"]).all()
    miss = cp["prim_id"] == cr.NO_PRIM
    assert miss.sum() >= 2 and np.isinf(near["dist2"][miss]).all(), "misses (the NaN and the inf point at least) are {+inf, NO_PRIM}"
    assert not bounded or name == "triangle" or (~miss).any()


# ---- 3. ties against the shrinking bound ----
@pytest.mark.parametrize("name", ["cube", "monkey"])
def test_ties_against_the_shrinking_bound(pkg, scenes, name):
    sd, sc = scenes(name)
    vq = cr.vertex_queries(sd, 512, 41)
    a, b, c = cr.tri_verts(sd)
    for k in (1, 2, 3):
        tree = sc.nearest_triangles(vq, k)  # (no counts: the bound shrinks to the slot's largest dist2, here 0)
        brute, _ = sc.list_neighbors_brute(vq, k=k)
        assert nr.same(tree, brute), (name, k, nr.first_difference(tree, brute))
        for i in range(0, 512, 37):
            sharing = np.flatnonzero((a == vq[i]).all(1) | (b == vq[i]).all(1) | (c == vq[i]).all(1))
            assert len(sharing) >= 3
            assert (tree[i]["dist2"] == 0).all() and tree[i]["prim_id"].tolist() == sharing[:k].tolist(), \
                "the k smallest prim_ids among the dist2 == 0 ties (a strict cull would lose the ones that arrive late)"


# ---- 4. with and without counts ----
@pytest.mark.parametrize("name", ["cornell", "blob"])
def test_with_and_without_counts(pkg, scenes, name):
    sd, sc = scenes(name)
    q = _q(sd, name)[:1024]
    for r2 in (INF, _r2(sd, 0.05)):
        counts = sc.count_neighbors(q, max_dist2=r2)
        for k in KS:
            plain = sc.nearest_triangles(q, k, max_dist2=r2)
            rec, c = sc.nearest_triangles(q, k, max_dist2=r2, want_counts=True)
            assert nr.same(plain, rec), (name, k, nr.first_difference(plain, rec))
            assert c.dtype == np.uint32 and (c == counts).all()
    finite = np.isfinite(q).all(axis=1)
    assert (sc.count_neighbors(q)[finite] == sd.ntris).all(), "unbounded: every triangle is a neighbour"


# ---- 5. per-query radii ----
def _mixed_radii(sd, n, seed):
    rng = np.random.default_rng(seed)
    r = _r2(sd, 0.05)
    choices = np.array([0.0, 1e-12 * r, r, np.inf, np.nan, -1.0], np.float32)
    return choices[rng.integers(0, len(choices), n)]


def test_per_query_radii(pkg, scenes):
    sd, sc = scenes("blob")
    q = _q(sd, "blob")
    radii = _mixed_radii(sd, NMAX, 5)
    radii[5], radii[6] = np.inf, np.inf  # the NaN and the inf point, under an unbounded radius
    ref = nr.neighbors(sd, q, radii)
    want_counts = np.diff(ref[0]).astype(np.uint32)
    counts = sc.count_neighbors(q, radii)
    assert (counts == want_counts).all(), np.flatnonzero(counts != want_counts)[:4]
    dead = np.isnan(radii) | (radii < 0)
    assert dead.sum() > 100 and (counts[dead] == 0).all() and counts[5] == 0 and counts[6] == 0
    assert (counts[np.isinf(radii) & np.isfinite(q).all(axis=1)] == sd.ntris).all()
    for k in (3,):
        want = nr.nearest(ref, k)
        got, c = sc.nearest_triangles(q, k, radii, want_counts=True)
        assert nr.same(got, want), nr.first_difference(got, want)
        assert (c == want_counts).all()
        assert nr.same(sc.nearest_triangles(q, k, radii), want)
        assert (got[dead] == nr.UNUSED).all() and (got[5] == nr.UNUSED).all() and (got[6] == nr.UNUSED).all(), "all-unused slots"
    # the full list: a short prefix (an unbounded query lists every triangle)
    m = 257
    off, rec = sc.list_neighbors(q[:m], radii[:m])
    pre = _prefix(ref, m)
    assert (off == pre[0]).all() and nr.same(rec, pre[1]), nr.first_difference(rec, pre[1])
    boff, brec = sc.list_neighbors_brute(q[:m], radii[:m])
    assert (boff == pre[0]).all() and nr.same(brec, pre[1])
    # the scalar max_dist2 is still checked where radii are given
    with pytest.raises(pkg.CgrtError):
        sc.count_neighbors(q, radii, max_dist2=float("nan"))


# ---- 6. configurations ----
def _tree_equals_brute(sc, q, r2):
    """count, full list and k slots of sc's tree search against its own brute force."""
    off, rec = sc.list_neighbors(q, max_dist2=r2)
    boff, brec = sc.list_neighbors_brute(q, max_dist2=r2)
    assert (off == boff).all() and nr.same(rec, brec), nr.first_difference(rec, brec)
    assert (sc.count_neighbors(q, max_dist2=r2) == np.diff(boff)).all()
    for k in (1, 8):
        tree = sc.nearest_triangles(q, k)  # (unbounded: the shrinking bound does all the culling)
        brute, _ = sc.list_neighbors_brute(q, k=k)
        assert nr.same(tree, brute), (k, nr.first_difference(tree, brute))
    return boff, brec


def test_linear_leaves(pkg, scenes):
    sd, accel = scenes("dodge")
    q = _q(sd, "dodge")[:1024]
    try:
        pkg.set_leaf_accel(False)
        sc = pkg.Scene(sd, device=0)
    finally:
        pkg.set_leaf_accel(True)
    try:
        assert sc.num_subnodes() == 0 and accel.num_subnodes() > 0
        r2 = _r2(sd, 0.02)
        boff, brec = _tree_equals_brute(sc, q, r2)
        off, rec = accel.list_neighbors(q, max_dist2=r2)
        assert (off == boff).all() and nr.same(rec, brec), "with and without in-leaf accelerators"
    finally:
        sc.close()


def test_long_runs_and_deep_accelerators(pkg):
    """The scene of test_closest_gpu.py::test_long_runs_and_deep_accelerators: leaves of ~34 triangles, accelerators three levels deep
    under two triangles per run, runs of 17 and more records under 32 per run."""
    sd = pkg.scenes.make_blob(70000, seed=3)
    q = cr.mixed_queries(sd, 1024, 13)
    r2 = _r2(sd, 0.02)
    want = None
    for run in (0, 32):
        try:
            pkg.set_leaf_accel(True, run)
            sc = pkg.Scene(sd, device=0)
        finally:
            pkg.set_leaf_accel(True)
        try:
            assert sc.num_subnodes() > 0
            got = _tree_equals_brute(sc, q, r2)
            assert want is None or ((got[0] == want[0]).all() and nr.same(got[1], want[1]))
            want = got
        finally:
            sc.close()


def test_nan_and_inf_vertices(pkg, scenes):
    clean, _ = scenes("blob")
    pos = np.asarray(clean.pos_nrm, np.float32).reshape(-1, 6).copy()
    tri = np.asarray(clean.tri).reshape(-1, 3)
    pos[tri[100, 1], 0] = np.nan
    pos[tri[900, 2], 1] = np.inf
    sd = dataclasses.replace(clean, pos_nrm=pos, name="blob+nan+inf")
    q = _q(clean, "blob")[:1024]
    sc = pkg.Scene(sd, device=0)
    try:
        r2 = _r2(clean, 0.05)
        boff, brec = _tree_equals_brute(sc, q, r2)
        ref = nr.neighbors(sd, q, None, r2)
        assert (boff == ref[0]).all() and nr.same(brec, ref[1]), nr.first_difference(brec, ref[1])
        everything, _ = sc.list_neighbors_brute(q[:64], k=sd.ntris)
        assert (everything["prim_id"] != 100).all(), "a triangle with a NaN coordinate is never listed"
        tree = sc.nearest_triangles(q[:64], sd.ntris)
        assert nr.same(tree, everything)
    finally:
        sc.close()


def test_empty_and_ignored_geometry(pkg, scenes, scene_data):
    sd = scene_data("spheres")
    assert sd.ntris == 0 and len(sd.spheres) > 0
    sc = pkg.Scene(sd, device=0)
    try:
        q = np.random.default_rng(3).normal(size=(130, 3)).astype(np.float32)
        assert not sc.count_neighbors(q).any()
        off, rec = sc.list_neighbors(q)
        assert not off.any() and len(rec) == 0
        for got in (sc.nearest_triangles(q, 3), sc.list_neighbors_brute(q, k=3)[0]):
            assert got.shape == (130, 3) and (got == nr.UNUSED).all()
        assert sc.debug_neighbor_work(q) == (0, 0) and sc.debug_neighbor_work(q, k=2) == (0, 0)
    finally:
        sc.close()
    sd, plain = scenes("blob")
    hi = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3].max(0)
    sph = np.asarray([[hi[0], hi[1], 0.0, 0.45 * hi[0], -1], [-hi[0], 0.0, hi[2], 0.4 * hi[0], 0]], np.float32)
    sc = pkg.Scene(dataclasses.replace(sd, spheres=sph, name="blob+spheres"), device=0)
    try:
        q, r2 = _q(sd, "blob")[:1024], _r2(sd, 0.05)
        ref = _prefix(_reference(sd, "blob", 0.05), 1024)
        off, rec = sc.list_neighbors(q, max_dist2=r2)
        assert (off == ref[0]).all() and nr.same(rec, ref[1]), "spheres beside the mesh are ignored"
        assert nr.same(sc.nearest_triangles(q, 3), plain.nearest_triangles(q, 3))
    finally:
        sc.close()


# ---- 7. the device forms ----
@pytest.mark.parametrize("n", LENGTHS)
def test_device_forms_between_guards_on_a_side_stream(pkg, scenes, n):
    sd, sc = scenes("blob")
    q, r2 = _q(sd, "blob")[:n], _r2(sd, 0.05)
    ref = _prefix(_reference(sd, "blob", 0.05), n)
    want_counts = np.diff(ref[0]).astype(np.int32)
    d_q = torch.from_numpy(q.copy()).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    # counts
    gc = Guarded(4 * n)
    out_c = gc.tensor((n,), torch.int32)
    assert sc.count_neighbors_tensor(d_q, r2, out=out_c, stream=side) is out_c
    side.synchronize()
    assert gc.intact() and (out_c.cpu().numpy() == want_counts).all()
    # k slots, with counts
    k = 3
    gr, gk = Guarded(8 * n * k), Guarded(4 * n)
    out_r = gr.tensor((n, k, 2))
    d_counts = gk.tensor((n,), torch.int32)
    sc.list_neighbors_device(d_q.data_ptr(), n, out_r.data_ptr(), n * k, k=k, d_counts_ptr=d_counts.data_ptr(), max_dist2=r2,
                             stream=side.cuda_stream)
    side.synchronize()
    assert gr.intact() and gk.intact()
    assert nr.same(_records(out_r), nr.nearest(ref, k)) and (d_counts.cpu().numpy() == want_counts).all()
    rec = sc.nearest_triangles_tensor(d_q, k, r2, out=out_r, stream=side)
    side.synchronize()
    assert rec is out_r and gr.intact() and nr.same(_records(out_r), nr.nearest(ref, k))
    rec, cnt = sc.nearest_triangles_tensor(d_q, k, max_dist2=r2, want_counts=True)
    assert nr.same(_records(rec), nr.nearest(ref, k)) and cnt.dtype == torch.int32 and (cnt.cpu().numpy() == want_counts).all()
    # offsets: the full list between guards
    m = int(ref[0][-1])
    go = Guarded(8 * max(m, 1))
    out_o = go.tensor((max(m, 1), 2))
    d_off = torch.from_numpy(ref[0].astype(np.int64)).cuda()
    side.wait_stream(torch.cuda.current_stream())
    if m:
        sc.list_neighbors_device(d_q.data_ptr(), n, out_o.data_ptr(), m, d_offsets_ptr=d_off.data_ptr(), max_dist2=r2, stream=side.cuda_stream)
    side.synchronize()
    assert go.intact()
    if m:
        assert nr.same(_records(out_o), ref[1])
    off, recs = sc.list_neighbors_tensor(d_q, r2, stream=side)
    side.synchronize()
    assert off.dtype == torch.int64 and (off.cpu().numpy() == ref[0]).all() and nr.same(_records(recs), ref[1])
    # per-query radii as a tensor
    radii = _mixed_radii(sd, n, 9)
    d_rad = torch.from_numpy(radii).cuda()
    full = nr.neighbors(sd, q, radii)
    got = sc.nearest_triangles_tensor(d_q, k, d_rad)
    assert nr.same(_records(got), nr.nearest(full, k))
    assert (sc.count_neighbors_tensor(d_q, d_rad).cpu().numpy() == np.diff(full[0])).all()
    with pytest.raises(ValueError):
        sc.nearest_triangles_tensor(d_q, k, out=torch.zeros((n, k + 1, 2), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        sc.count_neighbors_tensor(d_q.cpu())
    with pytest.raises(ValueError):
        sc.count_neighbors_tensor(d_q, torch.zeros(n + 1, dtype=torch.float32, device="cuda"))


def test_hostile_offsets(pkg, scenes):
    """The device form never reads the offsets on the host: a decreasing pair is an empty slot, both ends are clamped to capacity."""
    sd, sc = scenes("cube")
    a, _, _ = cr.tri_verts(sd)
    corner = a[0]
    pts = np.stack([corner, corner, corner, corner]).astype(np.float32)
    full = nr.neighbors(sd, pts, None, 0.0)
    capacity = 6
    offsets = np.array([4, 7, 1, 3, 3], np.uint64)  # [4, 7) cut to [4, 6); [7, 1): empty; [1, 3); [3, 3): empty
    g = Guarded(8 * (capacity + 10))  # ten more records than the call may write
    buf = g.tensor((capacity + 10, 2))
    d_q, d_off = torch.from_numpy(pts).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()
    before = _records(buf).copy()
    sc.list_neighbors_device(d_q.data_ptr(), 4, buf.data_ptr(), capacity, d_offsets_ptr=d_off.data_ptr(), max_dist2=0.0)
    torch.cuda.synchronize()
    got = _records(buf)
    want = nr.fill_slots(full, before[:capacity].copy(), offsets=offsets)
    assert g.intact() and nr.same(got[capacity:], before[capacity:]), "nothing beyond the first `capacity` records"
    assert nr.same(got[:capacity], want), (got[:capacity], want)
    assert nr.same(got[[0, 3]], before[[0, 3]]), "records no slot owns keep their bytes"
    # ends far beyond capacity, with counts
    offsets = np.array([0, 1 << 40, 1 << 41, (1 << 41) + 5, 1 << 62], np.uint64)
    d_off = torch.from_numpy(offsets.view(np.int64)).cuda()
    d_counts = torch.zeros(4, dtype=torch.int32, device="cuda")
    sc.list_neighbors_device(d_q.data_ptr(), 4, buf.data_ptr(), capacity, d_offsets_ptr=d_off.data_ptr(), d_counts_ptr=d_counts.data_ptr(),
                             max_dist2=0.0)
    torch.cuda.synchronize()
    got = _records(buf)
    tied = int(full[0][1])
    assert g.intact() and nr.same(got[capacity:], before[capacity:])
    assert nr.same(got[:capacity], nr.fill_slots(full, before[:capacity].copy(), offsets=offsets))
    assert (d_counts.cpu().numpy() == tied).all(), "the counts are the full numbers whatever the slots hold"


def test_device_forms_check_their_buffers(pkg, scenes):
    sd, sc = scenes("cube")
    n, k = 16, 2
    d_q = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    d_o = torch.zeros((n, k, 2), dtype=torch.float32, device="cuda")
    d_c = torch.zeros((n,), dtype=torch.int32, device="cuda")
    d_r = torch.ones((n,), dtype=torch.float32, device="cuda")
    d_off = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    host = np.zeros((n, k, 2), np.float32)
    host_off = np.zeros(n + 1, np.uint64)
    sc.count_neighbors_device(d_q.data_ptr(), n, d_c.data_ptr(), d_radius2_ptr=d_r.data_ptr())
    sc.list_neighbors_device(d_q.data_ptr(), n, d_o.data_ptr(), n * k, k=k, d_counts_ptr=d_c.data_ptr())
    sc.list_neighbors_device(d_q.data_ptr(), n, d_o.data_ptr(), n * k, d_offsets_ptr=d_off.data_ptr())
    torch.cuda.synchronize()
    bad = [lambda: sc.count_neighbors_device(d_q.data_ptr(), n, host.ctypes.data),
           lambda: sc.count_neighbors_device(host.ctypes.data, n, d_c.data_ptr()),
           lambda: sc.count_neighbors_device(d_q.data_ptr(), n, d_c.data_ptr(), d_radius2_ptr=host.ctypes.data),
           lambda: sc.list_neighbors_device(d_q.data_ptr(), n, host.ctypes.data, n * k, k=k),
           lambda: sc.list_neighbors_device(d_q.data_ptr(), n, d_o.data_ptr(), n * k, d_offsets_ptr=host_off.ctypes.data),
           lambda: sc.list_neighbors_device(d_q.data_ptr(), n, d_o.data_ptr(), n * k, k=k, d_counts_ptr=host.ctypes.data),
           lambda: sc.count_neighbors_device(d_q.data_ptr(), n, d_c.data_ptr(), max_dist2=float("nan"))]
    for f in bad:
        with pytest.raises(pkg.CgrtError) as e:
            f()
        assert e.value.code == -1
    sc.count_neighbors_device(0, 0, 0)  # n == 0 touches nothing
    sc.list_neighbors_device(0, 0, 0, 0, k=1)


def test_four_threads_on_one_scene(pkg, scenes):
    sd, sc = scenes("blob")
    q, r2 = _q(sd, "blob"), _r2(sd, 0.05)
    radii = _mixed_radii(sd, NMAX, 5)

    def one():
        off, rec = sc.list_neighbors(q, max_dist2=r2)
        near, c = sc.nearest_triangles(q, 3, radii, want_counts=True)
        return off.tobytes() + rec.tobytes() + near.tobytes() + c.tobytes()

    single = one()
    results, errors = [None] * 4, []

    def work(j):
        try:
            for _ in range(2):
                results[j] = one()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(r == single for r in results), "the host forms are concurrent on one scene"


# ---- 8. the bound shrinks ----
def test_work_on_dodge(pkg, scenes):
    sd, sc = scenes("dodge")
    q = cr.surface_queries(sd, 4096, 51)
    nodes, tris = sc.debug_neighbor_work(q, k=8)
    print(f"dodge, {len(q)} on-surface queries, k = 8, unbounded: {nodes / len(q):.1f} node steps and {tris / len(q):.1f} triangles evaluated "
          f"per query of {sd.ntris}")
    assert nodes > 0 and tris >= 8 * len(q)
    assert tris < len(q) * sd.ntris / 2, tris / len(q)
    cn, ct = sc.debug_neighbor_work(q)
    assert ct == len(q) * sd.ntris, "the count search of an unbounded radius evaluates every triangle: its bound never shrinks"
    assert cn > 0

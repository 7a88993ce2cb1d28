"""GPU tests of the winding-number queries (include/cgrt.h cgrt_winding_numbers*; Scene.winding_numbers and its _device / _tensor / _brute /
grid forms, debug_winding_work, inside_winding_tensor, signed_distance_winding_tensor).

* Bytes.  The tree form at beta = +inf returns the brute entry's bytes, w and inside: on the first k triangles of blob for k around the
  cluster sizes (1, 7, 8, 9, 63, 64, 65, 512, 513), on cube, blob, dodge and the 20 000-triangle dragon, for 1 .. 4 097 points of
  closest_ref.mixed_queries (on the surface, at vertices, on edges, far, one NaN and one inf point), with the in-leaf accelerators and
  with linear leaves.  A range the stackless walk skipped or walked twice shows here.
* Work counters.  At beta = 2 and 4 the three counters equal those of tests/winding_ref.py walk: the f32 far decisions are the definition.
* Values.  At beta = 2 and 4, |w_dev - walk(float64)| <= 4 * max_i |walk(float32)_i - walk(float64)_i| (at least 2^-20), the right-hand
  side computed here on the same points; the same for the brute entry against brute(float64).  The factor 4: the device's atan2f and
  numpy's float32 arctan2 are different few-ulp implementations of one function over identical sums.  The figures are printed.
* Meaning.  On the open dodge and blob `inside` at beta = 2 equals |scale_ref.winding64| > 0.5 outside the band ||w64| - 0.5| < 0.05 (2 %
  of the points at most); on the closed cube and dragon signed_distance_winding_tensor equals sdf_tensor bit for bit at every point
  farther than 1e-4 extents from the surface.
* Forms.  Host, device (side stream, between guards) and tensor forms agree bytewise; a NULL output leaves the other's bytes as they are
  and a buffer not asked for keeps its sentinel; grids equal the list form on sdf_grid_points; non-finite points and a scene without
  meshes give 0 and 0; non-finite vertices neither fault nor hang; four threads on a fresh scene give the single-thread bytes and the
  tree is built and uploaded once."""
import dataclasses
import threading

import numpy as np
import pytest

import closest_ref as cr
import scale_ref as sr
import winding_ref as wr
from conftest import same_bits
from test_winding_cpu import TRUNCATIONS, truncated

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
INF = float("inf")
LENGTHS = (1, 63, 64, 65, 129, 4097)
NMAX = max(LENGTHS)
FIXTURES = ("cube", "blob", "dodge", "dragon")
NSIGN = 1025
FLOOR = 2.0 ** -20  # of the value bounds


class Guarded:
    """nbytes of device memory between two guards, all of it sentinel bytes before the call."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def tensor(self, dtype, shape):
        return self.buf[PAD : PAD + self.n].view(dtype).view(tuple(shape))

    def bytes(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[PAD : PAD + self.n]

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n :] == SENTINEL).all())


_scenes = {}
_walks = {}


def _data(pkg, scene_data, name):
    if name == "dragon":
        return pkg.scenes.make_dragon(20_000)
    if name.startswith("blob:"):
        return truncated(scene_data("blob"), int(name[5:]))
    return scene_data(name)


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    """name -> (SceneData, Scene on device 0), created once."""

    def get(name):
        if name not in _scenes:
            sd = _data(pkg, scene_data, name)
            _scenes[name] = (sd, pkg.Scene(sd, device=0))
        return _scenes[name]

    yield get
    for _, sc in _scenes.values():
        sc.close()
    _scenes.clear()
    _walks.clear()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, what):
    (gw, gi), (ww, wi) = got, want
    assert gw.dtype == np.float32 and gi.dtype == np.bool_ and gw.shape == ww.shape and gi.shape == wi.shape, what
    bad = np.flatnonzero(~same_bits(gw, ww).reshape(-1) | (gi != wi).reshape(-1))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), gw.reshape(-1)[bad[0]], ww.reshape(-1)[bad[0]])


def _sign_walk(sc, sd, name, beta):
    """The restatement on the scene's sign queries, once: (points, w in float64, w in float32, counters)."""
    if (name, beta) not in _walks:
        tree = sc.debug_winding_tree()
        recs = wr.records(sd, tree)
        q = sr.sign_queries(sd, NSIGN, 11)
        w64, work = wr.walk(tree, recs, q, beta, np.float64)
        w32, work32 = wr.walk(tree, recs, q, beta, np.float32)
        assert work == work32 and w32.dtype == np.float32
        _walks[(name, beta)] = (q, w64, w32, work)
    return _walks[(name, beta)]


# ---- 1. bytes: the tree form with no cluster far is the brute form ----
def _tree_is_brute(sc, q, what):
    for n in LENGTHS:
        p = q[:n]
        _same(sc.winding_numbers(p, beta=INF), sc.winding_numbers_brute(p), (what, n))
    w, i = sc.winding_numbers_brute(q)
    fin = np.isfinite(q).all(axis=1)
    assert (w[~fin] == 0).all() and not i[~fin].any()
    return w, i


@pytest.mark.parametrize("name", [f"blob:{k}" for k in TRUNCATIONS] + list(FIXTURES))
def test_tree_form_at_infinite_beta_returns_the_brute_bytes(pkg, scenes, name):
    sd, sc = scenes(name)
    q = cr.mixed_queries(sd, NMAX, 11)
    w, i = _tree_is_brute(sc, q, name)
    fin = np.isfinite(q).all(axis=1)
    assert np.isfinite(w[fin]).all()
    if name in FIXTURES:
        assert i.any() and (~i).any() and (np.abs(w[fin]) > 0.9).any() and (np.abs(w[fin]) < 0.1).any()
        # a threshold of its own, and a finite beta does change bytes (the comparison above is not vacuous)
        assert ((np.abs(w) > 0.25) == sc.winding_numbers_brute(q, threshold=0.25, want="inside")).all()
        if name != "cube":
            assert (sc.winding_numbers(q, beta=2.0, want="w").view(np.uint32) != w.view(np.uint32)).any()


@pytest.mark.parametrize("name", ["blob:513", "dodge"])
def test_linear_leaves(pkg, scenes, name):
    sd, accel = scenes(name)
    q = cr.mixed_queries(sd, NMAX, 11)
    try:
        pkg.set_leaf_accel(False)
        sc = pkg.Scene(sd, device=0)
    finally:
        pkg.set_leaf_accel(True)
    try:
        assert sc.num_subnodes() == 0
        _tree_is_brute(sc, q, (name, "linear leaves"))
        # another record order: other (fatter) clusters and another order of the additions, held to the same restatement
        tree = sc.debug_winding_tree()
        recs = wr.records(sd, tree)
        moved = int((tree["record_prims"] != accel.debug_winding_tree()["record_prims"]).sum())
        print(f"{name}: {moved} of {len(recs)} records lie elsewhere without the in-leaf accelerators")
        qs = sr.sign_queries(sd, 129, 11)
        assert sc.debug_winding_work(qs, beta=2.0) == wr.walk(tree, recs, qs, 2.0, np.float32)[1]
        b64, b32 = wr.brute(recs, qs, np.float64), wr.brute(recs, qs, np.float32)
        scale = max(float(np.abs(b32.astype(np.float64) - b64).max()), FLOOR)
        assert np.abs(sc.winding_numbers_brute(qs, want="w").astype(np.float64) - b64).max() <= 4 * scale
    finally:
        sc.close()


# ---- 2. the work counters are the restatement's ----
@pytest.mark.parametrize("beta", [2.0, 4.0])
@pytest.mark.parametrize("name", FIXTURES)
def test_work_counters(pkg, scenes, name, beta):
    sd, sc = scenes(name)
    q, _, _, work = _sign_walk(sc, sd, name, beta)
    got = sc.debug_winding_work(q, beta=beta)
    print(f"{name} beta {beta}: per point {got[0] / len(q):.1f} clusters tested, {got[1] / len(q):.1f} dipoles, {got[2] / len(q):.1f} triangles")
    assert got == work, (name, beta, got, work)
    assert sc.debug_winding_work(q, beta=INF) == (len(q) * len(sc.debug_winding_tree()["clusters"]), 0, len(q) * sd.ntris)


# ---- 3. the values against the float64 walk ----


@pytest.mark.parametrize("beta", [2.0, 4.0])
@pytest.mark.parametrize("name", FIXTURES)
def test_tree_values(pkg, scenes, name, beta):
    sd, sc = scenes(name)
    q, w64, w32, _ = _sign_walk(sc, sd, name, beta)
    got = sc.winding_numbers(q, beta=beta, want="w")
    scale = max(float(np.abs(w32.astype(np.float64) - w64).max()), FLOOR)
    err = float(np.abs(got.astype(np.float64) - w64).max())
    print(f"{name} beta {beta}: max |dev - walk64| {err:.3e}, max |walk32 - walk64| {scale:.3e}, ratio {err / scale:.2f}; "
          f"device bytes equal to walk32 at {100.0 * (got.view(np.uint32) == w32.view(np.uint32)).mean():.1f} % of the points")
    assert scale <= 1e-3, "the float32 restatement itself is sound on these points (none on the surface)"
    assert err <= 4 * scale, (name, beta, err, scale)


@pytest.mark.parametrize("name", FIXTURES)
def test_brute_values(pkg, scenes, name):
    sd, sc = scenes(name)
    tree = sc.debug_winding_tree()
    recs = wr.records(sd, tree)
    q = sr.sign_queries(sd, 129, 11)
    b64, b32 = wr.brute(recs, q, np.float64), wr.brute(recs, q, np.float32)
    got = sc.winding_numbers_brute(q, want="w")
    scale = max(float(np.abs(b32.astype(np.float64) - b64).max()), FLOOR)
    err = float(np.abs(got.astype(np.float64) - b64).max())
    print(f"{name} brute: max |dev - brute64| {err:.3e}, max |brute32 - brute64| {scale:.3e}, ratio {err / scale:.2f}")
    assert scale <= 1e-3
    assert err <= 4 * scale, (name, err, scale)
    assert np.abs(b64 - sr.winding64(sd, q)).max() <= 1e-12, "the restatement is the float64 winding number"


# ---- 4. meaning ----
@pytest.mark.parametrize("name", ["dodge", "blob"])
def test_inside_on_open_meshes_is_the_float64_verdict(pkg, scenes, name):
    sd, sc = scenes(name)
    assert not sr.is_closed(sd)
    q = sr.sign_queries(sd, NSIGN, 11)
    w64 = sr.winding64(sd, q)
    keep = np.abs(np.abs(w64) - 0.5) >= 0.05
    truth = np.abs(w64) > 0.5
    inside = _np(sc.inside_winding_tensor(torch.from_numpy(q).cuda(), beta=2.0))
    print(f"{name}: {100.0 * (~keep).mean():.2f} % in the band, {100.0 * truth.mean():.1f} % inside, "
          f"{int((inside != truth)[keep].sum())} verdicts differ outside the band")
    assert (~keep).sum() <= 0.02 * len(q)
    assert truth[keep].any() and (~truth[keep]).any()
    assert (inside[keep] == truth[keep]).all(), int((inside != truth)[keep].sum())
    assert (inside == sc.winding_numbers(q, beta=2.0, want="inside")).all()


@pytest.mark.parametrize("name", ["cube", "dragon"])
def test_signed_distance_on_closed_meshes_is_sdf_tensor(pkg, scenes, name):
    sd, sc = scenes(name)
    assert sr.is_closed(sd)
    q = sr.sign_queries(sd, 513, 11)
    keep = cr.dist64(sd, q).min(axis=1) > 1e-4 * sr.extent(sd)
    d_q = torch.from_numpy(q).cuda()
    want = _np(sc.sdf_tensor(d_q, want="sdf"))
    got = _np(sc.signed_distance_winding_tensor(d_q))
    assert (~keep).sum() <= 0.02 * len(q) and (want[keep] < 0).any() and (want[keep] > 0).any()
    assert got.dtype == np.float32 and (got.view(np.uint32)[keep] == want.view(np.uint32)[keep]).all(), int((got != want)[keep].sum())
    bounded = _np(sc.signed_distance_winding_tensor(d_q, max_dist2=(0.5e-4 * sr.extent(sd)) ** 2))  # (below every kept point's distance)
    assert np.isinf(bounded[keep]).all() and (np.signbit(bounded[keep]) == (want[keep] < 0)).all(), "beyond max_dist2: +-inf with the sign"


# ---- 5. forms ----
@pytest.mark.parametrize("n", (1, 65, 4097))
def test_host_device_and_tensor_forms_agree(pkg, scenes, n):
    sd, sc = scenes("blob")
    q = cr.mixed_queries(sd, NMAX, 11)[:n]
    host = sc.winding_numbers(q)
    d_q = torch.from_numpy(q.copy()).cuda()
    g_w, g_i = Guarded(4 * n), Guarded(n)
    out_w, out_i = g_w.tensor(torch.float32, (n,)), g_i.tensor(torch.bool, (n,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    w, i = sc.winding_numbers_tensor(d_q, out=(out_w, out_i), stream=side)
    side.synchronize()
    assert w is out_w and i is out_i, "out= is returned as passed"
    assert g_w.intact() and g_i.intact()
    _same((_np(w), _np(i)), host, ("tensor form on a side stream", n))
    assert set(np.unique(g_i.bytes())) <= {0, 1}
    r_w, r_i = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    sc.winding_numbers_device(d_q.data_ptr(), n, r_w.data_ptr(), r_i.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    _same((_np(r_w), _np(r_i).view(np.bool_)), host, ("raw device form", n))
    # one output NULL: the other's bytes are what they were, a buffer that was not asked for keeps its sentinel
    o_w, o_i = Guarded(4 * n), Guarded(n)
    only_w = sc.winding_numbers_tensor(d_q, want="w", out=o_w.tensor(torch.float32, (n,)))
    assert _np(only_w).tobytes() == host[0].tobytes() and (o_i.bytes() == SENTINEL).all() and o_w.intact()
    only_i = sc.winding_numbers_tensor(d_q, want="inside", out=o_i.tensor(torch.bool, (n,)))
    assert (_np(only_i) == host[1]).all() and o_i.intact() and _np(only_w).tobytes() == host[0].tobytes() and o_w.intact()
    assert sc.winding_numbers(q, want="w").tobytes() == host[0].tobytes() and (sc.winding_numbers(q, want="inside") == host[1]).all()
    with pytest.raises(ValueError):
        sc.winding_numbers_tensor(d_q, out=(torch.zeros(n + 1, dtype=torch.float32, device="cuda"), out_i))
    with pytest.raises(ValueError):
        sc.winding_numbers_tensor(d_q.cpu())


def test_device_form_checks_its_buffers(pkg, scenes):
    sd, sc = scenes("cube")
    d_q = torch.zeros((16, 3), dtype=torch.float32, device="cuda")
    d_w = torch.full((16,), 7.0, dtype=torch.float32, device="cuda")
    d_i = torch.full((16,), 9, dtype=torch.uint8, device="cuda")
    host = np.zeros(64, np.float32)
    for args in ((host.ctypes.data, 16, d_w.data_ptr(), d_i.data_ptr()), (d_q.data_ptr(), 16, host.ctypes.data, d_i.data_ptr()),
                 (d_q.data_ptr(), 16, d_w.data_ptr(), host.ctypes.data)):
        with pytest.raises(pkg.CgrtError) as e:
            sc.winding_numbers_device(*args)
        assert e.value.code == -1, args
    with pytest.raises(pkg.CgrtError) as e:
        sc.winding_grid_device((0, 0, 0), (1, 1, 1), (4, 2, 2), host.ctypes.data, d_i.data_ptr())
    assert e.value.code == -1
    with pytest.raises(pkg.CgrtError) as e:
        sc.winding_numbers_device(d_q.data_ptr(), 16, d_w.data_ptr(), d_i.data_ptr(), beta=0.5)
    assert e.value.code == -1
    assert (_np(d_w) == 7.0).all() and (_np(d_i) == 9).all(), "refused before any work"
    sc.winding_numbers_device(0, 0, d_w.data_ptr(), 0)  # n == 0 touches nothing
    assert (_np(d_w) == 7.0).all()


GRID_DIMS = ((1, 1, 1), (9, 4, 5), (3, 70, 2))


@pytest.mark.parametrize("name", ["cube", "blob"])
def test_grids(pkg, scenes, name):
    sd, sc = scenes(name)
    lo, hi = cr.scene_box(sd)
    ext = hi - lo
    cases = [(tuple(lo - 0.15 * ext), tuple(1.3 * ext / np.maximum(np.asarray(d) - 1, 1)), d) for d in GRID_DIMS]
    cases.append((tuple(hi + 0.1 * ext), (-0.11 * ext[0], 0.0, 0.3 * ext[2]), (9, 4, 5)))  # negative and zero spacing
    for origin, spacing, dims in cases:
        for beta in (2.0, INF):
            nx, ny, nz = dims
            pts = pkg.sdf_grid_points(origin, spacing, dims)
            want = sc.winding_numbers(pts, beta=beta)
            g_w, g_i = Guarded(4 * len(pts)), Guarded(len(pts))
            w, i = sc.winding_grid_tensor(origin, spacing, dims, beta=beta,
                                          out=(g_w.tensor(torch.float32, (nz, ny, nx)), g_i.tensor(torch.bool, (nz, ny, nx))))
            got = (_np(w), _np(i))
            assert got[0].shape == (nz, ny, nx) and g_w.intact() and g_i.intact(), dims
            _same((got[0].reshape(-1), got[1].reshape(-1)), want, (dims, beta, "grid against the list form on sdf_grid_points"))
            host = sc.winding_grid(origin, spacing, dims, beta=beta)
            assert host[0].shape == (nz, ny, nx) and host[1].shape == (nz, ny, nx)
            _same(host, got, (dims, beta, "host grid form against the device grid form"))
            assert (_np(sc.winding_grid_tensor(origin, spacing, dims, beta=beta, want="inside")) == got[1]).all()


def test_special_points(pkg, scenes):
    sd, sc = scenes("cube")
    lo, hi = cr.scene_box(sd)
    q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.inf, -np.inf], 0.5 * (lo + hi), hi + (hi - lo)], np.float32)
    forms = ((sc.winding_numbers, 0.05), (sc.winding_numbers_brute, 1e-5), (lambda p: sc.winding_numbers(p, beta=INF), 1e-5),
             (lambda p: tuple(_np(x) for x in sc.winding_numbers_tensor(torch.from_numpy(p).cuda())), 0.05))
    for f, tol in forms:  # (tol: every triangle, or the dipoles of beta = 2)
        w, i = f(q)
        assert (w[:4] == 0).all() and not np.signbit(w[:4]).any() and not i[:4].any(), "non-finite points: 0 and 0, no walk"
        assert abs(abs(w[4]) - 1) < tol and i[4] and abs(w[5]) < tol and not i[5], "the cube's centre, and a point outside"
    assert sc.debug_winding_work(q[:4]) == (0, 0, 0)


def test_a_scene_without_meshes(pkg, scene_data):
    sd = scene_data("spheres")
    assert sd.ntris == 0 and len(sd.spheres) > 0
    sc = pkg.Scene(sd, device=0)
    try:
        q = np.random.default_rng(3).normal(size=(130, 3)).astype(np.float32)
        before = sc.device_bytes()
        for w, i in (sc.winding_numbers(q), sc.winding_numbers(q, beta=INF), sc.winding_numbers_brute(q),
                     sc.winding_grid((-1, -1, -1), (0.5, 0.5, 0.5), (5, 4, 3))):
            assert (w == 0).all() and not np.signbit(w).any() and not i.any()
        assert sc.debug_winding_work(q) == (0, 0, 0) and sc.device_bytes() == before
        t = sc.debug_winding_tree()
        assert len(t["clusters"]) == 0 and list(t["level_offsets"]) == [0]
    finally:
        sc.close()


def test_non_finite_vertices_neither_fault_nor_hang(pkg, scenes):
    clean, _ = scenes("blob")
    pos = np.asarray(clean.pos_nrm, np.float32).reshape(-1, 6).copy()
    tri = np.asarray(clean.tri).reshape(-1, 3)
    pos[tri[100, 1], 0] = np.nan
    pos[tri[900, 2], 1] = np.inf
    sd = dataclasses.replace(clean, pos_nrm=pos, name="blob+nan+inf")
    q = cr.mixed_queries(clean, 1024, 11)
    sc = pkg.Scene(sd, device=0)
    try:
        for beta in (2.0, INF):
            w, i = sc.winding_numbers(q, beta=beta)
            assert not i[np.isnan(w)].any(), "a NaN is not inside"
        _same(sc.winding_numbers(q, beta=INF), sc.winding_numbers_brute(q), "blob+nan+inf")
        tree = sc.debug_winding_tree()
        top = tree["clusters"][tree["level_offsets"][-2] :]
        assert not np.isfinite(top[:, 3]).all(), "a cluster over a NaN vertex has a NaN radius: it is never far"
        work = sc.debug_winding_work(q, beta=2.0)
        assert work == wr.walk(tree, wr.records(sd, tree), q, 2.0, np.float32)[1]
    finally:
        sc.close()


def test_four_threads_on_a_fresh_scene(pkg, scenes):
    sd, warm = scenes("blob")
    q = cr.mixed_queries(sd, NMAX, 11)
    single = tuple(x.tobytes() for x in warm.winding_numbers(q))
    sc = pkg.Scene(sd, device=0)
    try:
        before, h0 = sc.device_bytes(), sc.layout_hash()
        results, errors = [None] * 4, []
        start = threading.Barrier(4)

        def work(k):
            try:
                start.wait()
                for _ in range(3):
                    results[k] = tuple(x.tobytes() for x in sc.winding_numbers(q))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert all(r == single for r in results), "the host form is concurrent on one scene"
        nclusters = len(sc.debug_winding_tree()["clusters"])
        assert sc.device_bytes() == before + 32 * nclusters, "the tree is built and uploaded once"
        assert sc.layout_hash() == h0
        sc.winding_numbers_brute(q[:8])
        assert sc.device_bytes() == before + 32 * nclusters
    finally:
        sc.close()

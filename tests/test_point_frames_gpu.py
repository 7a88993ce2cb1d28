"""GPU: point-set frames (cgrt_point_frames*; include/cgrt.h "Point-set frames").  The yardstick is bit equality with the
numpy restatement (tests/point_frames_ref.py, whose own properties tests/test_point_frames_cpu.py holds): no margin.

The clouds (point_frames_ref.cloud, m = 2000; the surface samples m = 1500): a sphere shell with noise, a flat patch with duplicates, a
cloud offset by 100 with spread 0.01, a cloud with NaN and inf rows, and sample_surface points of the cube fixture.  Each is queried by
itself (skip_same_index, n = m: eight blocks, the last one partial) and by a separate list of n = 300 (two blocks), under a radius that
holds about a dozen data points, so that at k = 33 most queries have used < k.  k in {1, 2, 3, 8, 33}.

 1  device form (PointGrid.frames), host form and brute form: the restatement's bytes, frames and neighbours alike; neighbours equal
    PointGrid.nearest on the same arguments
 2  three cell sizes a factor of 16 apart and two streams: the same bytes
 3  per-query radius2 with NaN, negative, 0 and +inf entries
 4  orient flips exactly the records the definition says and leaves tangent_u alone; float64 determinant > 0.99 wherever used >= 3 and the
    eigenvalues are distinct
 5  used of 0, 1 and 2; m = 0; n = 0; squares that overflow (NaN stored as 0x7fc00000)
 6  data, queries, cell and bound scaled by 2^+-8 and 2^+-40 inside the envelope: centroid x 2^s, eigenvalues x 2^2s, the rest unchanged
 7  knn_frames equals the brute form at r2 = +inf, also on a cloud with fewer than k points
 8  the tensor views alias one buffer"""
import numpy as np
import pytest

import point_frames_ref as fref
import point_neighbors_ref as nref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INF = float("inf")
KS = (1, 2, 3, 8, 33)
CLOUDS = ("shell", "patch", "offset", "holes", "surface")


@pytest.fixture(scope="module")
def sc(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=0)
    yield s
    s.close()


_clouds = {}


def _cloud(sc, name):
    """(data, separate queries, r2: the squared radius that holds about a dozen data points), computed once, never changed."""
    if name not in _clouds:
        if name == "surface":
            data = sc.sample_surface_tensor(1500, seed=21)["point"].contiguous().cpu().numpy()
            pts = (data[:300] + np.float32(0.01) * np.random.default_rng(4).normal(size=(300, 3)).astype(np.float32)).astype(np.float32)
        else:
            data, pts = fref.cloud(name, m=2000, n=300)
        d2 = nref.d2_matrix(pts[np.isfinite(pts).all(1)][:64], data[np.isfinite(data).all(1)])
        r2 = np.float32(np.median(np.partition(d2, 12, axis=1)[:, 12]))
        for a in (data, pts):
            a.setflags(write=False)
        _clouds[name] = (data, pts, float(r2))
    return _clouds[name]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def _words(x):
    """Frame records of any form as (n, 16) uint32, neighbour records as (n * k, 2) uint32."""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    frames = x.dtype.itemsize == 64 or (x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 16)  # (neighbour tensors are (n, k, 2))
    return x.view(np.uint32).reshape(-1, 16 if frames else 2)


def _same(got, want, what):
    got, want = _words(got), _words(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} records differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}")


def _device(sc, data, pts, k, cell, grid=None, **kw):
    grid = grid or sc.point_grid_tensor(_t(data), cell)
    tkw = dict(kw)
    for key in ("radius2", "orient"):
        if isinstance(tkw.get(key), np.ndarray):
            tkw[key] = _t(tkw[key])
    return grid.frames(_t(pts), _t(data), k, **tkw)


# ---- 1 ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CLOUDS)
def test_all_forms_give_the_restatements_bytes(sc, name, k):
    data, pts, r2 = _cloud(sc, name)
    cell = float(np.sqrt(r2))
    grid = sc.point_grid_tensor(_t(data), cell)
    for q, skip in ((data, True), (pts, False)):
        want, slots = fref.frames(q, data, k, max_dist2=r2, skip_same_index=skip)
        used = want["used"]
        print(f"{name} k={k} n={len(q)}: used 0/1/2/k: {(used == 0).sum()} {(used == 1).sum()} {(used == 2).sum()} {(used == k).sum()}")
        kw = dict(max_dist2=r2, skip_same_index=skip)
        res = _device(sc, data, q, k, cell, grid=grid, **kw)
        _same(res["records"], want, "device frames")
        _same(res["neighbors"], slots, "device neighbours")
        _same(res["neighbors"], grid.nearest(_t(q), k, **kw), "neighbours against PointGrid.nearest")
        fr, nb = sc.point_frames(data, cell, q, k, want_neighbors=True, **kw)
        _same(fr, want, "host frames")
        _same(nb, slots, "host neighbours")
        _same(sc.point_frames(data, cell, q, k, **kw), want, "host frames without neighbours")
        fr, nb = sc.point_frames_brute(data, q, k, want_neighbors=True, **kw)
        _same(fr, want, "brute frames")
        _same(nb, slots, "brute neighbours")


# ---- 2 ----
def test_cell_and_stream_do_not_matter(sc):
    data, pts, r2 = _cloud(sc, "shell")
    want, slots = fref.frames(pts, data, 8, max_dist2=r2)
    tp, td = _t(pts), _t(data)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i, f in enumerate((1 / 16, 1.0, 16.0)):
        grid = sc.point_grid_tensor(td, float(np.sqrt(r2)) * f)
        torch.cuda.synchronize()
        out = [grid.frames(tp, td, 8, max_dist2=r2, stream=s) for s in streams]
        torch.cuda.synchronize()
        for res in out:
            _same(res["records"], want, f"cell x {f}")
            _same(res["neighbors"], slots, f"cell x {f}: neighbours")
        _same(sc.point_frames(data, float(np.sqrt(r2)) * f, pts, 8, max_dist2=r2), want, f"host form, cell x {f}")


# ---- 3 ----
def test_per_query_radius(sc):
    data, pts, r2 = _cloud(sc, "holes")
    rad = np.full(len(pts), r2, np.float32)
    rad[0::5], rad[1::5], rad[2::5], rad[3::5] = np.nan, -1.0, 0.0, np.inf
    q = pts.copy()
    q[2::10] = data[2 : 2 + len(q[2::10])]  # (r2 = 0 finds coincident points only)
    want, slots = fref.frames(q, data, 8, radius2=rad)
    assert (want["used"][0::5] == 0).all() and (want["used"][1::5] == 0).all() and (want["used"][2::10] >= 1).any()
    res = _device(sc, data, q, 8, float(np.sqrt(r2)), radius2=rad)
    _same(res["records"], want, "device frames")
    _same(res["neighbors"], slots, "device neighbours")
    _same(sc.point_frames(data, float(np.sqrt(r2)), q, 8, radius2=rad), want, "host frames")
    _same(sc.point_frames_brute(data, q, 8, radius2=rad), want, "brute frames")


# ---- 4 ----
def test_orientation_and_handedness(sc):
    data, pts, r2 = _cloud(sc, "shell")
    o = (-pts).astype(np.float32)  # (towards the centre of the shell)
    o[::7, 1] = np.nan
    o[3::7, 2] = np.inf
    plain, slots = fref.frames(pts, data, 8, max_dist2=r2)
    want, _ = fref.frames(pts, data, 8, max_dist2=r2, orient=o, slots=slots)
    res = _device(sc, data, pts, 8, float(np.sqrt(r2)), max_dist2=r2, orient=o)
    _same(res["records"], want, "device frames")
    _same(sc.point_frames(data, float(np.sqrt(r2)), pts, 8, max_dist2=r2, orient=o), want, "host frames")
    _same(sc.point_frames_brute(data, pts, 8, max_dist2=r2, orient=o), want, "brute frames")
    got = res["records"].cpu().numpy().view(fref.FRAME).reshape(-1)
    flip = np.isfinite(o).all(1) & (fref._dot(plain["normal"], o) < 0) & (plain["used"] > 0)
    assert 50 < flip.sum() < len(pts) - 50
    assert np.array_equal(got["normal"][flip], -plain["normal"][flip]) and np.array_equal(got["normal"][~flip], plain["normal"][~flip])
    assert np.array_equal(got["tangent_u"], plain["tangent_u"])
    assert np.array_equal(got["tangent_v"][flip], -plain["tangent_v"][flip])
    lam = np.stack([got["lambda0"], got["lambda1"], got["lambda2"]], 1)
    distinct = (got["used"] >= 3) & (lam[:, 0] < lam[:, 1]) & (lam[:, 1] < lam[:, 2])
    F = np.stack([got["normal"], got["tangent_u"], got["tangent_v"]], 1).astype(np.float64)
    assert distinct.sum() > 100 and (np.linalg.det(F[distinct]) > 0.99).all()


# ---- 5 ----
def test_degenerate_neighbourhoods_and_empty_calls(sc, pkg):
    data = np.float32([[0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5], [np.nan, 0, 0]])
    pts = np.float32([[0.1, 0, 0], [5, 5, 5.5], [40, 40, 40], [np.inf, 0, 0], [0.4, 0.8, 0]])
    for k, r2 in ((4, 1.5), (2, INF), (1, INF), (3, 0.3)):
        want, slots = fref.frames(pts, data, k, max_dist2=r2)
        res = _device(sc, data, pts, k, 1.0, max_dist2=r2)
        _same(res["records"], want, f"device frames k={k}")
        _same(res["neighbors"], slots, f"device neighbours k={k}")
        _same(sc.point_frames(data, 1.0, pts, k, max_dist2=r2), want, f"host frames k={k}")
        _same(sc.point_frames_brute(data, pts, k, max_dist2=r2), want, f"brute frames k={k}")
    want, _ = fref.frames(pts, data, 4, max_dist2=1.5)
    assert sorted(set(want["used"].tolist())) == [0, 1, 2]
    # no data, no queries
    empty = np.zeros((0, 3), np.float32)
    for d, q in ((empty, pts), (data, empty), (empty, empty)):
        want, slots = fref.frames(q, d, 3)
        assert not want.view(np.uint8).any()
        res = _device(sc, d, q, 3, 1.0)
        assert res["records"].shape == (len(q), 16) and res["neighbors"].shape == (len(q), 3, 2) and res["eigenvalues"].shape == (len(q), 3)
        _same(res["records"], want, "device frames")
        _same(res["neighbors"], slots, "device neighbours")
        fr, nb = sc.point_frames(d, 1.0, q, 3, want_neighbors=True)
        _same(fr, want, "host frames")
        _same(nb, slots, "host neighbours")
        _same(sc.point_frames_brute(d, q, 3), want, "brute frames")
    # e e overflows: inf, then NaN, stored as the canonical one
    big = np.ldexp(np.random.default_rng(2).random((300, 3)).astype(np.float32), 100)
    want, slots = fref.frames(big[:70], big, 6)
    assert np.isnan(want["lambda2"]).any()
    res = _device(sc, big, big[:70], 6, float(2.0**98))
    _same(res["records"], want, "device frames, overflow")
    _same(sc.point_frames_brute(big, big[:70], 6), want, "brute frames, overflow")


# ---- 6 ----
@pytest.mark.parametrize("s", [-40, -8, 8, 40])
def test_scale_relations_are_exact(sc, s):
    base, q0 = fref.scale_case(s)
    e = fref.SCALE_CASES[s]
    cell0, r20 = float(2.0 ** (e - 3)), float(2.0 ** (2 * e - 5))  # (a ball of radius 2^-2.5 edges holds about 28 of the 1200 points)
    want0, slots0, det0 = fref.frames(q0, base, 8, max_dist2=r20, skip_same_index=True, detail=True)
    ok = fref.in_frame_envelope(det0, s) & (want0["used"] == 8)
    assert ok.mean() >= 0.5, "the envelope leaves too few queries for the case to show anything"
    g0 = _device(sc, base, q0, 8, cell0, max_dist2=r20, skip_same_index=True)
    _same(g0["records"], want0, "scale 1")
    gs = _device(sc, np.ldexp(base, s), np.ldexp(q0, s), 8, float(np.ldexp(cell0, s)), max_dist2=float(np.ldexp(r20, 2 * s)), skip_same_index=True)
    a = g0["records"].cpu().numpy().view(fref.FRAME).reshape(-1)[ok]
    b = gs["records"].cpu().numpy().view(fref.FRAME).reshape(-1)[ok]
    assert np.array_equal(a["used"], b["used"])
    for f in ("normal", "tangent_u", "tangent_v"):
        assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f
    assert np.array_equal(np.ldexp(a["centroid"], s).view(np.uint32), b["centroid"].view(np.uint32))
    for f in ("lambda0", "lambda1", "lambda2"):
        assert np.array_equal(np.ldexp(a[f], 2 * s).view(np.uint32), b[f].view(np.uint32)), f
    n0 = g0["neighbors"].cpu().numpy().view(np.uint32)[ok.nonzero()[0]]
    ns = gs["neighbors"].cpu().numpy().view(np.uint32)[ok.nonzero()[0]]
    assert np.array_equal(n0[..., 1], ns[..., 1])
    assert np.array_equal(np.ldexp(n0[..., 0].view(np.float32), 2 * s).view(np.uint32), ns[..., 0])


# ---- 7 ----
@pytest.mark.parametrize("k", [1, 8, 33])
def test_knn_frames_equal_the_brute_form(sc, k):
    rng = np.random.default_rng(12)
    centres = rng.random((12, 3))
    data = (centres[rng.integers(0, 12, 1500)] + 0.01 * rng.normal(size=(1500, 3))).astype(np.float32)  # clustered: several doublings
    pts = rng.random((300, 3)).astype(np.float32)
    o = rng.normal(size=(300, 3)).astype(np.float32)
    grid = sc.point_grid_tensor(_t(data), 0.01)
    for q, skip, orient in ((pts, False, o), (data, True, None)):
        want, slots = sc.point_frames_brute(data, q, k, skip_same_index=skip, orient=orient, want_neighbors=True)
        res = grid.knn_frames(_t(q), _t(data), k, skip_same_index=skip, orient=None if orient is None else _t(orient))
        _same(res["records"], want, "knn_frames")
        _same(res["neighbors"], slots, "knn_frames neighbours")
        assert (want["used"] == k).all()
    few = data[: k - 1] if k > 1 else data[:0]
    want, slots = sc.point_frames_brute(few, pts, k, want_neighbors=True)
    res = sc.point_grid_tensor(_t(few), 0.05).knn_frames(_t(pts), _t(few), k)
    _same(res["records"], want, "knn_frames on fewer than k points")
    _same(res["neighbors"], slots, "knn_frames neighbours on fewer than k points")
    assert (want["used"] == len(few)).all()


# ---- 8 ----
def test_views_alias_one_buffer(sc):
    data, pts, r2 = _cloud(sc, "shell")
    res = _device(sc, data, pts, 8, float(np.sqrt(r2)), max_dist2=r2)
    rec = res["records"]
    assert rec.shape == (len(pts), 16) and rec.dtype == torch.float32 and res["used"].dtype == torch.int32
    base, span = rec.data_ptr(), rec.numel() * 4
    for key, col, shape in (("centroid", 0, (len(pts), 3)), ("used", 3, (len(pts),)), ("normal", 4, (len(pts), 3)), ("eigenvalues", 7, (len(pts), 3)),
                            ("tangent_u", 8, (len(pts), 3)), ("tangent_v", 12, (len(pts), 3))):
        v = res[key]
        assert tuple(v.shape) == shape and v.data_ptr() == base + 4 * col and base <= v.data_ptr() < base + span, key
    assert res["eigenvalues"].stride() == (16, 4)
    assert torch.equal(res["eigenvalues"][:, 1], rec[:, 11]) and torch.equal(res["used"], rec.view(torch.int32)[:, 3])
    assert res["neighbors"].shape == (len(pts), 8, 2)

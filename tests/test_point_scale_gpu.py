"""GPU tests of the point queries across scale: closest points, crossing counts and lists, the fused signed distance (include/cgrt.h
"Envelope" paragraphs).  Scene, query points and ray origins are multiplied by 2^k, k in KS.

* Bit parity at EVERY k, inside and outside the envelope: the header's promise -- tree search == device brute force == the restatement,
  every operation rounded, nothing contracted, denormals preserved -- among denormal products, inf - inf, NaN in the clamp and `inf > inf`
  in the cull.  cube and blob against tests/closest_ref.py, crossings_ref.py and sdf_ref.py; dodge (in-leaf accelerators) and the 20 k
  dragon, too large for all pairs on the CPU, tree against device brute force on 257 queries and the fused kernel against the composition
  of signed_distance_tensor and inside_tensor.  Host, tensor and grid forms; max_dist2 = +inf, FLT_MAX and ldexp(r^2, 2k).  The runs at
  2^62 and 2^-70 are asserted to hold non-finite and denormal dist2.
* Covariance on the device: wherever scale_ref.in_envelope says yes, the device's results at 2^k are the exact power-of-two images of its
  results at 1, for every record; the work counters of the closest search and all five of the fused kernel over those queries are equal
  too (the search order and the early end of the vote are scale-free).  This needs no CPU reference, so dodge and the dragon get a
  check that is not "the device against itself through the same functions".  k = 30 is inside the envelope for the near query families
  and every ray family but the camera's on all four scenes, k = -20 for cube, blob and
  dragon; dodge has sliver triangles ((2 * area)^2 = 2^-68) whose |cross|^2 is subnormal at 2^-20 -- the restatement itself is not
  covariant there -- so dodge is swept at 2^-10 as well, which is inside.
* Truth on a curved closed mesh: the fused kernel's sign against the float64 winding number and its distance against the float64
  referee on the 20 k dragon, with and without in-leaf accelerators."""
import numpy as np
import pytest

import closest_ref as cr
import crossings_ref as xr
import scale_ref as sr
import sdf_ref
from conftest import same_bits
from test_closest_cpu import K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = (-70, -31, -20, 0, 30, 33, 62)
EXTRA_KS = {"dodge": (-10,)}
SMALL, LARGE = ("cube", "blob"), ("dodge", "dragon")
N, N_BRUTE = 1025, 257
LIST_CAP = 64
SEED = 11
INF = float("inf")
GRIDS = ((9, 4, 5), (3, 70, 2))
FAR = 4  # closest_ref.mixed_queries: query i belongs to family i % 5, the far family is the last
CAMERA = 0  # crossings_ref.mixed_rays: ray i belongs to family i % 7, the camera's rays are the first

_data = {}
_scenes = {}


@pytest.fixture(scope="module")
def world(pkg, orc, scene_data):
    """get(name, k) -> (scaled SceneData, Scene on device 0, scaled queries, scaled rays), each made once."""

    def data(name):
        if name not in _data:
            sd = pkg.scenes.make_dragon(20_000) if name == "dragon" else scene_data(name)
            _data[name] = (sd, cr.mixed_queries(sd, N, SEED), xr.mixed_rays(pkg, orc, sd, N, SEED))
        return _data[name]

    def get(name, k):
        sd, q, rays = data(name)
        if (name, k) not in _scenes:
            sk = sr.scaled(sd, k)
            _scenes[(name, k)] = (sk, pkg.Scene(sk, device=0))
        sk, sc = _scenes[(name, k)]
        return sk, sc, sr.scaled_points(q, k), sr.scaled_rays(rays, k)

    yield get
    for _, sc in _scenes.values():
        sc.close()
    _scenes.clear()


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_closest(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool((a["prim_id"] == b["prim_id"]).all()) and all(bool(same_bits(a[f], b[f]).all()) for f in ("point", "dist2", "bary"))


def _first_closest(a, b):
    for i in range(min(len(a), len(b))):
        if not _same_closest(a[i : i + 1], b[i : i + 1]):
            return i, a[i], b[i]
    return None


def _same_crossings(a, b):
    """CROSSING_DTYPE arrays: ids equal, t bit for bit with a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.shape == b.shape and bool((a["prim_id"] == b["prim_id"]).all()) and bool(same_bits(a["t"], b["t"]).all())


def _first_crossing(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    if a.shape != b.shape:
        return "shapes", a.shape, b.shape
    d = np.flatnonzero((a["prim_id"] != b["prim_id"]) | ~same_bits(a["t"], b["t"]))
    return None if len(d) == 0 else (int(d[0]), a[d[0]], b[d[0]])


def _assert_sdf(got, want, what, rows=None):
    (gs, gi), (ws, wi) = got, want
    gs, gi, ws, wi = (np.asarray(x).reshape(-1) for x in (gs, gi, ws, wi))
    if rows is not None:
        gs, gi, ws, wi = gs[rows], gi[rows], ws[rows], wi[rows]
    assert gs.dtype == np.float32 and gi.dtype == np.bool_ and gs.shape == ws.shape and gi.shape == wi.shape, what
    bad = np.flatnonzero(~same_bits(gs, ws) | (gi != wi))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), gs[bad[0]], ws[bad[0]], gi[bad[0]], wi[bad[0]])


def _radii(sd0, k):
    """max_dist2 of the sweep: +inf, FLT_MAX and ldexp(r^2, 2k) with r a quarter of the unscaled scene's size, where that is finite."""
    r2 = np.float32((0.25 * cr.scene_scale(sd0)) ** 2)
    with np.errstate(all="ignore"):
        rk = float(np.ldexp(r2, 2 * k))
    return (INF, sr.FLT_MAX) + ((rk,) if np.isfinite(rk) else ())


def _grids(sd0, k):
    """Grids over the unscaled scene's box grown by 15 %, origin and spacing (float32) multiplied by 2^k."""
    lo, hi = cr.scene_box(sd0)
    ext = hi - lo
    for dims in GRIDS:
        spacing = (1.3 * ext / np.maximum(np.asarray(dims) - 1, 1)).astype(np.float32)
        origin = (lo - 0.15 * ext).astype(np.float32)
        with np.errstate(all="ignore"):
            yield tuple(float(x) for x in np.ldexp(origin, k)), tuple(float(x) for x in np.ldexp(spacing, k)), dims


def _composition(sc, d_q, max_dist2=INF):
    inside = sc.inside_tensor(d_q)
    dist = torch.sqrt(sc.closest_points_tensor(d_q, max_dist2=max_dist2)["dist2"])
    return _np(torch.where(inside, -dist, dist)), _np(inside)


def _assert_edge_reached(k, q, rec):
    fin = np.isfinite(q).all(axis=1)
    d2 = rec["dist2"][fin]
    if k == 62:
        assert (~np.isfinite(d2)).any(), "the sweep reaches non-finite dist2 of finite queries at 2^62"
        assert (np.isposinf(d2) & (rec["prim_id"][fin] != cr.NO_PRIM)).any(), "+inf dist2 qualifies under an infinite radius"
    if k == -70:
        assert ((d2 > 0) & (d2 < sr.FLT_MIN)).any(), "the sweep reaches denormal dist2 at 2^-70"


# ---- 1. bit parity at every k: cube and blob against the restatements ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SMALL)
def test_parity_with_the_restatements(pkg, orc, world, name, k):
    sd0 = world(name, 0)[0]
    sd, sc, q, rays = world(name, k)
    d_q = torch.from_numpy(q.copy()).cuda()
    # closest points: tree == brute == restatement, host and tensor forms, three radii
    for md in _radii(sd0, k):
        ref = cr.brute(sd, q, md)
        tree, brute = sc.closest_points(q, md), sc.closest_points_brute(q, md)
        assert _same_closest(brute, ref), (name, k, md, "brute force against the restatement", _first_closest(brute, ref))
        assert _same_closest(tree, brute), (name, k, md, "tree search against brute force", _first_closest(tree, brute))
        ten = _np(sc.closest_points_tensor(d_q, max_dist2=md)["out"]).view(pkg.CLOSEST_DTYPE).reshape(-1)
        assert _same_closest(ten, tree), (name, k, md, "tensor form", _first_closest(ten, tree))
        assert not np.isnan(tree["dist2"][tree["prim_id"] != cr.NO_PRIM]).any(), "a NaN never qualifies"
        if md == INF:
            _assert_edge_reached(k, q, tree)
        # the fused kernel under the same radius
        want = sdf_ref.reference(orc, sd, q, pkg.INSIDE_DIRECTIONS, md)
        got = tuple(_np(x) for x in sc.sdf_tensor(d_q, max_dist2=md))
        _assert_sdf(got, want, (name, k, md, "fused kernel against the reference"))
        _assert_sdf(sc.sdf(q, max_dist2=md), got, (name, k, md, "host form against the tensor form"))
    # crossings: counts, full lists and first-2 slots
    counts, offsets, rec = ref_x = xr.reference(orc, sd, rays)
    assert (sc.count_crossings(rays) == counts).all(), (name, k, "counts")
    off_t, rec_t = sc.list_crossings(rays)
    off_b, rec_b = sc.list_crossings_brute(rays)
    assert (off_b == offsets).all() and _same_crossings(rec_b, rec), (name, k, "brute force list", _first_crossing(rec_b, rec))
    assert (off_t == offsets).all() and _same_crossings(rec_t, rec), (name, k, "tree search list", _first_crossing(rec_t, rec))
    f2, c2 = sc.first_crossings(rays, 2)
    assert (c2 == counts).all() and _same_crossings(f2, xr.first_k(ref_x, 2)), (name, k, "first two", _first_crossing(f2, xr.first_k(ref_x, 2)))
    d_r = torch.from_numpy(rays.copy()).cuda()
    assert (_np(sc.count_crossings_tensor(d_r)).view(np.uint32) == counts).all(), (name, k, "tensor counts")
    # grids: against the list form on sdf_grid_points and against the reference
    for origin, spacing, dims in _grids(sd0, k):
        nx, ny, nz = dims
        pts = pkg.sdf_grid_points(origin, spacing, dims)
        s, i = sc.sdf_grid_tensor(origin, spacing, dims)
        got = (_np(s), _np(i))
        assert got[0].shape == (nz, ny, nx)
        _assert_sdf(got, sc.sdf(pts), (name, k, dims, "grid against the list form on sdf_grid_points"))
        _assert_sdf(got, sdf_ref.reference(orc, sd, pts, pkg.INSIDE_DIRECTIONS), (name, k, dims, "grid against the reference"))
        _assert_sdf(sc.sdf_grid(origin, spacing, dims), got, (name, k, dims, "host grid form"))


# ---- 2. bit parity at every k: dodge and the dragon, tree against device brute force, fused against the composition ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", LARGE)
def test_parity_on_the_large_scenes(pkg, world, name, k):
    sd0 = world(name, 0)[0]
    sd, sc, q, rays = world(name, k)
    if k == 0:
        assert sc.num_subnodes() > 0, "dodge: the fixture with in-leaf accelerators; the dragon has them too"
    finite = np.isfinite(q).all(axis=1)
    d_q = torch.from_numpy(q.copy()).cuda()
    qb, rb = q[:N_BRUTE], np.ascontiguousarray(rays[:N_BRUTE])
    for md in _radii(sd0, k):
        tree, brute = sc.closest_points(qb, md), sc.closest_points_brute(qb, md)
        assert _same_closest(tree, brute), (name, k, md, "tree search against brute force", _first_closest(tree, brute))
        assert not np.isnan(tree["dist2"][tree["prim_id"] != cr.NO_PRIM]).any(), "a NaN never qualifies"
        full = sc.closest_points(q, md)
        assert _same_closest(full[:N_BRUTE], tree)
        ten = _np(sc.closest_points_tensor(d_q, max_dist2=md)["out"]).view(pkg.CLOSEST_DTYPE).reshape(-1)
        assert _same_closest(ten, full), (name, k, md, "tensor form", _first_closest(ten, full))
        if md == INF:
            _assert_edge_reached(k, q, full)
        got = tuple(_np(x) for x in sc.sdf_tensor(d_q, max_dist2=md))
        _assert_sdf(got, _composition(sc, d_q, md), (name, k, md, "fused kernel against the composition"), finite)
        _assert_sdf(sc.sdf(q, max_dist2=md), got, (name, k, md, "host form against the tensor form"))
        assert np.isposinf(got[0][~finite]).all() and not got[1][~finite].any()
    counts = sc.count_crossings(rb)
    ft, ct = sc.first_crossings(rb, 2)
    fb, cb = sc.list_crossings_brute(rb, k=2)
    assert (cb == counts).all() and (ct == counts).all(), (name, k, "counts of the tree search against brute force")
    assert _same_crossings(ft, fb), (name, k, "first two", _first_crossing(ft, fb))
    # the lists, each ray's slot as long as its count but at most LIST_CAP records: where the planes degenerate (2^62) every triangle is
    # a crossing of every ray at t = 0, and a slot's insertion sort is quadratic in its length
    slots = np.zeros(len(rb) + 1, np.int64)
    np.cumsum(np.minimum(counts, LIST_CAP), out=slots[1:])
    rec_t, ct = sc.list_crossings(rb, offsets=slots)
    rec_b, cb = sc.list_crossings_brute(rb, offsets=slots)
    assert (ct == counts).all() and (cb == counts).all() and _same_crossings(rec_t, rec_b), (name, k, "lists", _first_crossing(rec_t, rec_b))
    if k == 0:
        assert 2 <= counts.max() <= LIST_CAP, "at scale 1 the slots hold the full lists"
    for origin, spacing, dims in _grids(sd0, k):
        pts = pkg.sdf_grid_points(origin, spacing, dims)
        s, i = sc.sdf_grid_tensor(origin, spacing, dims)
        got = (_np(s), _np(i))
        _assert_sdf(got, sc.sdf(pts), (name, k, dims, "grid against the list form on sdf_grid_points"))
        _assert_sdf(sc.sdf_grid(origin, spacing, dims), got, (name, k, dims, "host grid form"))


# ---- 3. covariance on the device, and the work counters ----
def _device_results(sc, q, rays):
    off, rec = sc.list_crossings(rays)
    return dict(closest=sc.closest_points(q), crossings=(sc.count_crossings(rays), off, rec), first=sc.first_crossings(rays, 2)[0], sdf=sc.sdf(q))


def _work(sc, q):
    return sc.debug_closest_work(q), sc.debug_sdf_work(q)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_device_results_are_covariant_inside_the_envelope(pkg, world, name):
    sd0, sc0, q0, rays0 = world(name, 0)
    r0 = _device_results(sc0, q0, rays0)
    fin, rfin = np.isfinite(q0).all(axis=1), np.isfinite(rays0[:, 0:3]).all(axis=1)
    near = fin & (np.arange(N) % 5 != FAR)
    near_rays = rfin & (np.arange(N) % 7 != CAMERA)
    seen = {}
    for k in sorted(set(KS + EXTRA_KS.get(name, ())) - {0}):
        sd, sc, q, rays = world(name, k)
        env, renv = sr.in_envelope(sd, q), sr.in_envelope(sd, rays[:, 0:3])
        seen[k] = (env, renv)
        if not env.any() and not renv.any():
            continue
        rk = _device_results(sc, q, rays)
        for what, cov, inside in (("closest", sr.covariant_closest(r0["closest"], rk["closest"], k), env),
                                  ("crossings", sr.covariant_crossings(r0["crossings"], rk["crossings"], k), renv),
                                  ("first two crossings", sr.covariant_first(r0["first"], rk["first"], k), renv),
                                  ("sdf", sr.covariant_sdf(r0["sdf"], rk["sdf"], k), env)):
            bad = np.flatnonzero(inside & ~cov)
            assert len(bad) == 0, (name, k, what, "not covariant inside the envelope", len(bad), int(bad[0]))
        print(f"{name}, 2^{k}: {int(env.sum())} of {int(fin.sum())} queries and {int(renv.sum())} of {int(rfin.sum())} rays inside the envelope, all covariant")
        # the search order is scale-free: the same node steps and triangle evaluations over the queries inside the envelope
        sub0, subk = np.ascontiguousarray(q0[env]), np.ascontiguousarray(q[env])
        assert _work(sc, subk) == _work(sc0, sub0), (name, k, "work counters", _work(sc, subk), _work(sc0, sub0))
    assert seen[30][0][near].all() and seen[30][1][near_rays].all(), (name, "2^30 lies inside the envelope for the near families")
    low = -10 if name == "dodge" else -20
    assert seen[low][0][fin].all() and seen[low][1][rfin].all(), (name, low, "lies inside the envelope for every finite query and ray")


# ---- 4. truth on a curved closed mesh ----
@pytest.fixture(scope="module")
def dragon_truth(world):
    sd = world("dragon", 0)[0]
    assert sr.is_closed(sd)
    pts = sr.sign_queries(sd, 513, 61)
    return sd, pts, cr.dist64(sd, pts).min(axis=1), sr.winding64(sd, pts)


@pytest.mark.parametrize("accel", (True, False), ids=("accelerators", "linear leaves"))
def test_sign_and_distance_against_float64_on_the_dragon(pkg, world, dragon_truth, accel):
    sd, pts, D64, w = dragon_truth
    assert len(pts) == 513
    if accel:
        sc = world("dragon", 0)[1]
        assert sc.num_subnodes() > 0
    else:
        try:
            pkg.set_leaf_accel(False)
            sc = pkg.Scene(sd, device=0)
        finally:
            pkg.set_leaf_accel(True)
    try:
        assert accel or sc.num_subnodes() == 0
        s, i = sc.sdf_tensor(torch.from_numpy(pts.copy()).cuda())
        sdf, inside = _np(s), _np(i)
    finally:
        if not accel:
            sc.close()
    keep = D64 > 1e-4 * sr.extent(sd)
    truth = np.abs(w) > 0.5
    scale = np.maximum(1.0, np.maximum(np.abs(pts.astype(np.float64)).max(axis=1), cr.scene_scale(sd)))
    ratio = np.abs(np.abs(sdf.astype(np.float64)) - D64) / (2.0 ** -24 * scale)
    print(f"dragon 20 k: {100.0 * (~keep).mean():.2f} % left out, {100.0 * truth[keep].mean():.1f} % inside, largest ||sdf| - D64| "
          f"{ratio[keep].max():.3f} units (K = {K:.2f})")
    assert (~keep).sum() <= 0.02 * len(pts)
    assert (np.abs(np.abs(w[keep]) - truth[keep]) <= 1e-6).all()
    assert truth[keep].any() and (~truth[keep]).any()
    bad = np.flatnonzero(keep & (inside != truth))
    assert len(bad) == 0, (len(bad), int(bad[0]), pts[bad[0]], float(w[bad[0]]))
    assert (np.signbit(sdf) == inside).all()
    assert ratio[keep].max() <= K, (float(ratio[keep].max()), int(np.flatnonzero(keep)[ratio[keep].argmax()]))

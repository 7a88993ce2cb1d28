"""GPU tests of the host-pointer entries' one call helper (csrc/capi_lanes.cpp LaneCall: begin, input / scratch per slot, the launch,
output per result, finish; the queries reach it through QueryCall, one body for their host and device forms) through the entries written
with it.

A lane stages transfers of up to 1 MiB in pinned buffers -- a staged result reaches the caller's memory only in finish, behind the
stream -- and sends larger ones through the bounce buffers, in place when output returns.  Every entry below runs at N = 40 000 items,
where the ray upload (1.12 MB) and several results cross that limit while others of the same call stay staged, and in slices of 5 000,
where every transfer is staged.  The reference is the device-pointer form of the same entry on torch tensors of the same inputs (those
forms take no lane), byte for byte; entries without one are held to their concatenated slices.  Scene: the 2 000-triangle dragon stand-in.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 40_000
SLICE = 5_000
STAGE = 1 << 20  # capi_lanes.cpp kStageBytes
SENTINEL = np.float32(7.25)


@pytest.fixture(scope="module")
def world(pkg, orc):
    """The scene, N camera rays (hits and misses) with their hits from the device form, N points around the surface, two spherical lights,
    32 point lights, an 8-channel vertex table: made once, never written."""
    sd = pkg.scenes.make_dragon(2_000)
    sc = pkg.Scene(sd, device=0)
    W = H = 200
    rays = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    assert rays.shape == (N, 7) and rays.nbytes > STAGE
    rng = np.random.default_rng(40)
    pos = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, :3]
    lo, hi = pos.min(0), pos.max(0)
    points = (pos[rng.integers(0, len(pos), N)] + rng.normal(0, 0.05 * float((hi - lo).max()), (N, 3))).astype(np.float32)
    lights = np.concatenate([rng.uniform(lo - (hi - lo), hi + (hi - lo), (32, 3)), np.ones((32, 3))], 1).astype(np.float32)
    spherical = np.array([[*(hi + (hi - lo)), 1, 1, 1, 0.1], [*(lo - (hi - lo)), 1, 1, 1, 0.2]], np.float32)
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    sc.intersect_device(d_rays.data_ptr(), N, d_hits.data_ptr())
    torch.cuda.synchronize()
    hits = d_hits.cpu().numpy().view(pkg.HIT_DTYPE).reshape(N)
    assert hits["hit"].any() and not hits["hit"].all(), "the camera rays must hit and miss"
    attr = rng.standard_normal((len(pos), 8)).astype(np.float32)
    w = dict(pkg=pkg, sd=sd, sc=sc, rays=rays, hits=hits, points=points, lights=lights, spherical=spherical, units=pkg.unit_vector_table(4096, seed=3),
             attr=attr, d_rays=d_rays, d_hits=d_hits, d_points=torch.from_numpy(points).cuda(), d_attr=torch.from_numpy(attr).cuda())
    yield w
    sc.close()


@pytest.fixture(scope="module")
def fields(world):
    """What the neighbour, signed-distance and winding tests add to the world: per-query squared radii in [0, (0.1 extent)^2] with a few NaN
    and negative ones (slot 4 of the lane), and a 64 x 64 x 65 grid over the scene's box padded by 10 %, whose float plane (1 064 960 B)
    goes direct while its byte plane stays staged.  Made once, never written."""
    pos = np.asarray(world["sd"].pos_nrm, np.float32).reshape(-1, 6)[:, :3]
    lo, hi = pos.min(0), pos.max(0)
    extent = float((hi - lo).max())
    radius2 = np.random.default_rng(42).uniform(0, (0.1 * extent) ** 2, N).astype(np.float32)
    radius2[::1000], radius2[500::1000] = np.nan, -1.0
    dims = (64, 64, 65)
    grid = (lo - 0.1 * (hi - lo), 1.2 * (hi - lo) / (np.array(dims, np.float32) - 1), dims)
    assert dims[0] * dims[1] * dims[2] * 4 > STAGE > dims[0] * dims[1] * dims[2]
    return dict(radius2=radius2, d_radius2=torch.from_numpy(radius2).cuda(), max_dist2=(0.05 * extent) ** 2, grid=grid)


def _np(t):
    torch.cuda.synchronize()
    return np.ascontiguousarray(t.cpu().numpy())


def _slices(fn, n=N, step=SLICE):
    return [fn(slice(a, min(n, a + step))) for a in range(0, n, step)]


def _check(whole, device, parts, what):
    """whole: the host entry at N; device: the device form's bytes; parts: the host entry's slices."""
    whole = np.ascontiguousarray(whole)
    assert whole.tobytes() == np.ascontiguousarray(device).tobytes(), f"{what}: the host form at N differs from the device form"
    assert whole.tobytes() == np.concatenate([np.ascontiguousarray(p) for p in parts]).tobytes(), f"{what}: N at once differs from its slices"


def test_occluded(world):
    sc, rays = world["sc"], world["rays"]  # rays bounced, 40 KB of answers staged
    _check(sc.occluded(rays), _np(sc.occluded_tensor(world["d_rays"])), _slices(lambda s: sc.occluded(rays[s])), "occluded")


def test_occluded_with_answers_above_the_staging_limit(world):
    sc = world["sc"]
    n = 1_100_000  # one byte per answer: these too take the direct road
    assert n > STAGE
    rays = np.ascontiguousarray(np.resize(world["rays"], (n, 7)))
    got = sc.occluded(rays)
    assert got.tobytes() == _np(sc.occluded_tensor(torch.from_numpy(rays).cuda())).tobytes()
    assert got.any() and not got.all()


def test_in_shadow(world):
    sc, p, L = world["sc"], world["points"], world["lights"]  # 1.28 MB of answers direct, the points staged
    assert N * len(L) > STAGE > p.nbytes
    _check(sc.in_shadow(p, L), _np(sc.in_shadow_tensor(world["d_points"], L)), _slices(lambda s: sc.in_shadow(p[s], L)), "in_shadow")


def test_soft_lit(world):
    """(Sample smp of point i draws as pixel i of the call, so a slice is not the whole list's rows: each slice is held to the device form
    on the same slice.)"""
    sc, p, d_p, S, U = world["sc"], world["points"], world["d_points"], world["spherical"], world["units"]
    for s in [slice(0, N)] + [slice(a, a + SLICE) for a in range(0, N, SLICE)]:
        got = sc.soft_lit(p[s], S, U, samples=8, seed=5)
        assert got.nbytes <= STAGE and got.any() and not (got == 8).all()
        assert got.tobytes() == _np(sc.soft_lit_tensor(d_p[s], S, U, samples=8, seed=5)).tobytes(), s


@pytest.mark.parametrize("brute", [False, True])
def test_closest_points(world, brute):
    sc, p = world["sc"], world["points"]  # 1.28 MB of records direct
    f = sc.closest_points_brute if brute else sc.closest_points
    whole = f(p)
    assert whole.nbytes > STAGE
    parts = _slices(lambda s: f(p[s]))
    assert whole.tobytes() == np.concatenate(parts).tobytes()
    if not brute:  # (the brute force has no device form)
        assert whole.tobytes() == _np(sc.closest_points_tensor(world["d_points"])["out"]).tobytes()


def test_list_crossings_with_counts(world):
    """k = 4 and the counts asked for: the records (1.28 MB) are in place when their download returns while the counts (160 KB) wait,
    staged, for finish -- both kinds of result in one call."""
    sc, rays = world["sc"], world["rays"]
    rec, cnt = sc.first_crossings(rays, 4)
    assert rec.nbytes > STAGE > cnt.nbytes and cnt.any() and (cnt == 0).any()
    d_rec, d_cnt = sc.first_crossings_tensor(world["d_rays"], 4)
    assert rec.tobytes() == _np(d_rec).tobytes() and cnt.tobytes() == _np(d_cnt).tobytes()
    parts = _slices(lambda s: sc.first_crossings(rays[s], 4))
    assert rec.tobytes() == np.concatenate([r for r, _ in parts]).tobytes() and cnt.tobytes() == np.concatenate([c for _, c in parts]).tobytes()


def test_count_crossings(world):
    sc, rays = world["sc"], world["rays"]
    _check(sc.count_crossings(rays), _np(sc.count_crossings_tensor(world["d_rays"])), _slices(lambda s: sc.count_crossings(rays[s])), "count_crossings")


def test_interpolate_hits(world):
    sc, rays, hits, attr = world["sc"], world["rays"], world["hits"], world["attr"]  # 1.28 MB out direct, the hits staged
    whole = sc.interpolate_hits(rays, hits, attr)
    assert whole.nbytes > STAGE > hits.nbytes and whole.any()
    _check(whole, _np(sc.interpolate_hits_tensor(world["d_rays"], world["d_hits"], world["d_attr"])),
           _slices(lambda s: sc.interpolate_hits(rays[s], hits[s], attr)), "interpolate_hits")


def test_hit_barycentrics(world):
    sc, rays, hits = world["sc"], world["rays"], world["hits"]
    _check(sc.hit_barycentrics(rays, hits), _np(sc.hit_barycentrics_tensor(world["d_rays"], world["d_hits"])),
           _slices(lambda s: sc.hit_barycentrics(rays[s], hits[s])), "hit_barycentrics")


def test_interpolate_hits_grad(world):
    """Against the device form, 8 channels.  The order of the additions into one table element is unspecified, so bytes can only be
    compared where every order gives the same sum: grad_out is zero except for hits whose triangles share no vertex, and every table
    element then receives at most one non-zero product (x + 0 is x in any order).  The table starts from non-zero values, which have to
    go up for the sums to come out; all N rows of grad_out and hits go through the lane as in any other call."""
    sc, sd, rays, hits = world["sc"], world["sd"], world["rays"], world["hits"]
    tri = np.asarray(sd.tri).reshape(-1, 3)
    used, chosen = np.zeros(len(world["attr"]), bool), []
    for i in np.flatnonzero(hits["hit"]):
        v = tri[hits["prim_id"][i]]
        if not used[v].any():
            used[v] = True
            chosen.append(i)
    assert len(chosen) >= 10
    rng = np.random.default_rng(41)
    g = np.zeros((N, 8), np.float32)
    g[chosen] = rng.standard_normal((len(chosen), 8)).astype(np.float32)
    init = rng.standard_normal(world["attr"].shape).astype(np.float32)
    whole = sc.interpolate_hits_grad(rays, hits, g, grad_attr=init.copy())
    assert (whole != init).any()
    dev = sc.interpolate_hits_grad_tensor(world["d_rays"], world["d_hits"], torch.from_numpy(g).cuda(), grad_attr=torch.from_numpy(init).cuda())
    assert whole.tobytes() == _np(dev).tobytes()
    acc = init.copy()
    for a in range(0, N, SLICE):
        sc.interpolate_hits_grad(rays[a : a + SLICE], hits[a : a + SLICE], g[a : a + SLICE], grad_attr=acc)
    assert whole.tobytes() == acc.tobytes()


def test_intersect_batch_leaves_the_normals_of_misses(world):
    pkg, sc, rays = world["pkg"], world["sc"], world["rays"]

    def run(r):
        hits = np.zeros(len(r), pkg.HIT_DTYPE)
        normals = np.full((len(r), 3), SENTINEL, np.float32)
        pkg._check(pkg.lib().cgrt_intersect_batch(sc._h, pkg._ptr(r), len(r), pkg._ptr(hits), pkg._ptr(normals)))
        return hits, normals

    hits, normals = run(rays)
    miss = hits["hit"] == 0
    assert miss.any() and (~miss).any(), "the inputs must contain hits and misses"
    assert (normals[miss] == SENTINEL).all() and not (normals[~miss] == SENTINEL).all(axis=1).any()
    d_normals = torch.full((N, 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_hits = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    sc.intersect_device(world["d_rays"].data_ptr(), N, d_hits.data_ptr(), d_normals.data_ptr())
    assert hits.tobytes() == _np(d_hits).tobytes() and normals.tobytes() == _np(d_normals).tobytes()
    parts = _slices(lambda s: run(rays[s]))
    assert hits.tobytes() == np.concatenate([h for h, _ in parts]).tobytes() and normals.tobytes() == np.concatenate([n for _, n in parts]).tobytes()


def test_counted_entries_add_up_over_slices(world, fields):
    """cgrt_debug_closest_work, cgrt_debug_crossing_work, cgrt_debug_neighbor_work (the count search and the k-nearest search into records
    of the lane's own), cgrt_debug_sdf_work and cgrt_debug_winding_work (zero the lane's counters, a counted launch, the words back): the
    work of 5 000 items is the work of its slices of 1 000."""
    sc, p, rays, rad = world["sc"], world["points"][:5_000], world["rays"][17_500:22_500], fields["radius2"][:5_000]

    def parts(f):
        return _slices(f, 5_000, 1_000)

    for whole, part in ((sc.debug_closest_work(p), parts(lambda s: sc.debug_closest_work(p[s]))),
                        (sc.debug_crossing_work(rays), parts(lambda s: sc.debug_crossing_work(rays[s]))),
                        (sc.debug_neighbor_work(p, radius2=rad), parts(lambda s: sc.debug_neighbor_work(p[s], radius2=rad[s]))),
                        (sc.debug_neighbor_work(p, radius2=rad, k=8), parts(lambda s: sc.debug_neighbor_work(p[s], radius2=rad[s], k=8))),
                        (sc.debug_sdf_work(p), parts(lambda s: sc.debug_sdf_work(p[s]))),
                        (sc.debug_winding_work(p), parts(lambda s: sc.debug_winding_work(p[s])))):
        assert len(whole) in (2, 3, 5) and all(x > 0 for x in whole)
        assert whole == tuple(sum(col) for col in zip(*part))


def test_nearest_triangles_with_counts(world, fields):
    """k = 4 and the counts asked for, per-query radii: the records (1.28 MB) direct, the counts (160 KB) staged, the radii up through the
    lane's fifth slot."""
    sc, p, rad = world["sc"], world["points"], fields["radius2"]
    rec, cnt = sc.nearest_triangles(p, 4, radius2=rad, want_counts=True)
    assert rec.nbytes > STAGE > cnt.nbytes and (cnt == 0).any() and (cnt > 4).any() and ((cnt > 0) & (cnt < 4)).any()
    assert (cnt[::1000] == 0).all() and (cnt[500::1000] == 0).all(), "a NaN or negative radius has no neighbours"
    d_rec, d_cnt = sc.nearest_triangles_tensor(world["d_points"], 4, radius2=fields["d_radius2"], want_counts=True)
    assert rec.tobytes() == _np(d_rec).tobytes() and cnt.tobytes() == _np(d_cnt).tobytes()
    parts = _slices(lambda s: sc.nearest_triangles(p[s], 4, radius2=rad[s], want_counts=True))
    assert rec.tobytes() == np.concatenate([r for r, _ in parts]).tobytes() and cnt.tobytes() == np.concatenate([c for _, c in parts]).tobytes()


def test_count_neighbors(world, fields):
    sc, p, rad = world["sc"], world["points"], fields["radius2"]
    whole = sc.count_neighbors(p, radius2=rad)
    assert whole.any() and (whole == 0).any() and len(np.unique(whole)) > 2
    _check(whole, _np(sc.count_neighbors_tensor(world["d_points"], radius2=fields["d_radius2"])),
           _slices(lambda s: sc.count_neighbors(p[s], radius2=rad[s])), "count_neighbors")


def test_list_neighbors_in_full(world, fields):
    """The full lists under one radius: count, prefix sums, list; the offsets (320 KB) go up through slot 1, the records come down direct."""
    sc, p, r2 = world["sc"], world["points"], fields["max_dist2"]
    off, rec = sc.list_neighbors(p, max_dist2=r2)
    cnt = np.diff(off)
    assert rec.nbytes > STAGE > (N + 1) * 8 and len(rec) == off[-1] and (cnt == 0).any() and len(np.unique(cnt)) > 2
    d_off, d_rec = sc.list_neighbors_tensor(world["d_points"], max_dist2=r2)
    assert off.tobytes() == _np(d_off).tobytes() and rec.tobytes() == _np(d_rec).tobytes()
    parts = _slices(lambda s: sc.list_neighbors(p[s], max_dist2=r2))
    assert rec.tobytes() == np.concatenate([r for _, r in parts]).tobytes() and (cnt == np.concatenate([np.diff(o) for o, _ in parts])).all()


def test_list_crossings_in_full(world):
    """The full lists of the camera rays (the k form is above): the offsets through slot 1, as many records as the rays cross."""
    sc, rays = world["sc"], world["rays"]
    off, rec = sc.list_crossings(rays)
    cnt = np.diff(off)
    assert (N + 1) * 8 <= STAGE and len(rec) == off[-1] > 0 and (cnt == 0).any() and len(np.unique(cnt)) > 2
    d_off, d_rec = sc.list_crossings_tensor(world["d_rays"])
    assert off.tobytes() == _np(d_off).tobytes() and rec.tobytes() == _np(d_rec).tobytes()
    parts = _slices(lambda s: sc.list_crossings(rays[s]))
    assert rec.tobytes() == np.concatenate([r for _, r in parts]).tobytes() and (cnt == np.concatenate([np.diff(o) for o, _ in parts])).all()


def test_sdf(world):
    sc, p = world["sc"], world["points"]  # both outputs staged (160 KB and 40 KB)
    s, ins = sc.sdf(p)
    assert s.nbytes <= STAGE and ins.any() and not ins.all()
    d_s, d_ins = sc.sdf_tensor(world["d_points"])
    assert s.tobytes() == _np(d_s).tobytes() and ins.tobytes() == _np(d_ins).tobytes()
    parts = _slices(lambda q: sc.sdf(p[q]))
    assert s.tobytes() == np.concatenate([a for a, _ in parts]).tobytes() and ins.tobytes() == np.concatenate([b for _, b in parts]).tobytes()
    # inside alone: the lane's slot 1 is not used by the call
    _check(sc.sdf(p, want=("inside",)), ins, _slices(lambda q: sc.sdf(p[q], want=("inside",))), "sdf, inside alone")


def test_sdf_grid(world, fields):
    sc, (origin, spacing, dims) = world["sc"], fields["grid"]  # (a slab of the grid is another grid: no slices)
    s, ins = sc.sdf_grid(origin, spacing, dims)
    assert s.nbytes == 1_064_960 > STAGE > ins.nbytes and s.shape == ins.shape == dims[::-1] and ins.any() and not ins.all()
    d_s, d_ins = sc.sdf_grid_tensor(origin, spacing, dims)
    assert s.tobytes() == _np(d_s).tobytes() and ins.tobytes() == _np(d_ins).tobytes()


def test_winding_numbers(world, fields):
    sc, p = world["sc"], world["points"]  # the list staged; the grid's float plane direct, its byte plane staged
    w, ins = sc.winding_numbers(p)
    assert ins.any() and not ins.all()
    d_w, d_ins = sc.winding_numbers_tensor(world["d_points"])
    assert w.tobytes() == _np(d_w).tobytes() and ins.tobytes() == _np(d_ins).tobytes()
    parts = _slices(lambda q: sc.winding_numbers(p[q]))
    assert w.tobytes() == np.concatenate([a for a, _ in parts]).tobytes() and ins.tobytes() == np.concatenate([b for _, b in parts]).tobytes()
    origin, spacing, dims = fields["grid"]
    w, ins = sc.winding_grid(origin, spacing, dims)
    assert w.nbytes > STAGE > ins.nbytes and w.shape == ins.shape == dims[::-1] and ins.any() and not ins.all()
    d_w, d_ins = sc.winding_grid_tensor(origin, spacing, dims)
    assert w.tobytes() == _np(d_w).tobytes() and ins.tobytes() == _np(d_ins).tobytes()


@pytest.mark.parametrize("want_counts", [False, True])
def test_first_call_of_a_fresh_scene_lists_into_empty_slots(world, fields, want_counts):
    """A scene whose first host call is list_neighbors with every slot empty: without counts there is nothing to write and the call
    returns without a lane; with counts the lane is new and its records buffer is never sized."""
    pkg, p, r2 = world["pkg"], world["points"][:SLICE], fields["max_dist2"]
    sc = pkg.Scene(world["sd"], device=0)
    try:
        rec, cnt = sc.list_neighbors(p, max_dist2=r2, offsets=np.zeros(len(p) + 1, np.uint64), want_counts=want_counts)
        assert rec.shape == (0,) and rec.dtype == pkg.NEIGHBOR_DTYPE
        if want_counts:
            assert cnt.any() and (cnt == 0).any() and cnt.tobytes() == world["sc"].count_neighbors(p, max_dist2=r2).tobytes()
        else:
            assert cnt is None
    finally:
        sc.close()

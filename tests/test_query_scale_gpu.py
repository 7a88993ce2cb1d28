"""GPU tests of the neighbour and the winding-number queries across scale and on the large scenes (include/cgrt.h "Neighbour queries" and
"Winding numbers").  Scene and query points are multiplied by 2^k, k in KS (dodge also at 2^-10).

* Neighbour parity at EVERY k, inside and outside the envelope: tree search == device brute force == tests/neighbors_ref.py by bytes on
  cube and blob (1 025 closest_ref.mixed_queries), tree search == device brute force on dodge (in-leaf accelerators, slivers) and the
  20 000-triangle dragon (257 queries): counts, slots of min(count, 64) records through `offsets` with and without counts (without them
  the bound shrinks), nearest_triangles for k = 1 and 8; under the radii +inf, FLT_MAX, (0.05 extents)^2 * 2^2k and a per-query array
  cycling through 0.0, -0.0, a denormal, that radius, +inf, NaN and -1.  Asserted to be reached: counts above the 64-record cap at scale 1
  (the slots truncate), +inf dist2 that qualifies under the infinite radius and ties on prim_id at 2^62, denormal dist2 at 2^-70.
* Neighbour covariance: wherever scale_ref.in_envelope says yes the device's lists at 2^k are the power-of-two images of its lists at 1
  and debug_neighbor_work (count search, k = 8 search) is equal over the inside queries -- test_point_scale_gpu.py's assertions for the
  closest points, with its non-vacuity lines (2^30 for the near families; 2^-20, dodge 2^-10, for every finite query).
* Winding bytes at every k: the tree form at beta = +inf returns the brute form's bytes, w and inside, NaN and inf sums included (NaN w
  asserted at 2^62, inside 0 there); debug_winding_work at beta = 2 equals the float32 counters of tests/winding_ref.py; the grid form
  equals the list form on sdf_grid_points; non-finite points give +0.
* Winding inside scale_ref.in_winding_envelope (2^-20, 2^30, 2^33 on all four scenes, 2^-31 where test_query_scale_cpu.py found every
  point inside): the counters are those at scale 1; |w_dev - walk64| <= 4 * max(|walk32 - walk64|, 2^-20) with the right-hand side
  computed at that k (test_winding_gpu.py::test_tree_values' rule); `inside` is the verdict at scale 1 outside the band ||w64| - 0.5| <
  0.05 (2 % of the points at most).  The share of points whose device bits equal the device's at scale 1 is printed, not asserted:
  atan2f is not pinned by the definition.
* The dipole is IEEE: for the 129 far points at beta = 2 -- no triangle is evaluated, so every operation is +, -, *, / or sqrt -- the
  device's w equals winding_ref.walk(float32) bit for bit at every inside k.  A division or square root that is not correctly rounded,
  a contracted multiply-add or flushed denormals in k_winding's far branch fail here."""
import numpy as np
import pytest

import closest_ref as cr
import neighbors_ref as nr
import scale_ref as sr
import winding_ref as wr
from conftest import same_bits
from test_point_scale_gpu import _grids
from test_query_scale_cpu import INSIDE_LOW

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = (-70, -31, -20, 0, 30, 33, 62)
EXTRA_KS = {"dodge": (-10,)}
SMALL, LARGE = ("cube", "blob"), ("dodge", "dragon")
N, N_BRUTE = 1025, 257
LIST_CAP = 64
SEED = 11
RADIUS = 0.05  # of the extent
INF = float("inf")
FAR = 4  # closest_ref.mixed_queries: query i belongs to family i % 5, the far family is the last
NEAREST = (1, 8)
WINDING_INSIDE_KS = (-31, -20, 30, 33)
NFAR = 129
FLOOR = 2.0 ** -20  # test_winding_gpu.py: of the value bounds
BAND = 0.05

_data = {}
_scenes = {}
_w0 = {}


@pytest.fixture(scope="module")
def world(pkg, scene_data):
    """get(name, k) -> (scaled SceneData, Scene on device 0, scaled mixed queries), each made once; get.sign(name, k) and get.far(name, k):
    the scaled sign (1 025) and far queries of the winding tests, get.few(name, k): 257 sign queries."""

    def data(name):
        if name not in _data:
            sd = pkg.scenes.make_dragon(20_000) if name == "dragon" else scene_data(name)
            _data[name] = (sd, cr.mixed_queries(sd, N, SEED), sr.sign_queries(sd, N, SEED), cr.far_queries(sd, NFAR, 15),
                           sr.sign_queries(sd, N_BRUTE, SEED))
        return _data[name]

    def get(name, k):
        sd, q = data(name)[:2]
        if (name, k) not in _scenes:
            sk = sr.scaled(sd, k)
            _scenes[(name, k)] = (sk, pkg.Scene(sk, device=0))
        sk, sc = _scenes[(name, k)]
        return sk, sc, sr.scaled_points(q, k)

    get.sign = lambda name, k: sr.scaled_points(data(name)[2], k)
    get.far = lambda name, k: sr.scaled_points(data(name)[3], k)
    get.few = lambda name, k: sr.scaled_points(data(name)[4], k)
    yield get
    _w0.clear()
    for _, sc in _scenes.values():
        sc.close()
    _scenes.clear()


def _r2(sd0, k):
    """(0.05 extents)^2 of the unscaled scene times 2^2k, as float32 (0 or +inf where it leaves the range)."""
    with np.errstate(all="ignore"):
        return np.float32(np.ldexp(np.float32(np.float32(RADIUS * nr.extent(sd0)) ** 2), 2 * k))


def _bounds(sd0, k, n):
    """The bounds of the sweep as (label, radius2 array or None, max_dist2)."""
    rk = _r2(sd0, k)
    cycle = np.array([0.0, -0.0, 1e-42, rk, np.inf, np.nan, -1.0], np.float32)
    assert np.signbit(cycle[1]) and 0 < cycle[2] < sr.FLT_MIN
    out = [("+inf", None, INF), ("FLT_MAX", None, sr.FLT_MAX)]
    if np.isfinite(rk) and rk > 0:
        out.append(("radius", None, float(rk)))
    out.append(("per query", np.ascontiguousarray(cycle[np.arange(n) % len(cycle)]), INF))
    return out


def _slots(counts):
    slots = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.minimum(counts.astype(np.int64), LIST_CAP), out=slots[1:])
    return slots


def _device_answers(sc, q, radii, md, brute):
    """counts, capped slots with and without counts, and the k nearest, by the tree search or by the device's brute force."""
    if brute:
        _, counts = sc.list_neighbors_brute(q, radii, md, k=1)
    else:
        counts = sc.count_neighbors(q, radii, md)
    slots = _slots(counts)
    out = dict(counts=counts, slots=slots)
    if slots[-1] > 0:
        if brute:
            out["listed"], c = sc.list_neighbors_brute(q, radii, md, offsets=slots)
            out["plain"] = out["listed"]
        else:
            out["listed"], c = sc.list_neighbors(q, radii, md, offsets=slots, want_counts=True)
            out["plain"], none = sc.list_neighbors(q, radii, md, offsets=slots, want_counts=False)
            assert none is None
        assert (c == counts).all(), "the counts of a list call are the full numbers whatever the slots hold"
    else:
        out["listed"] = out["plain"] = np.zeros(0, nr.NEIGHBOR_DTYPE)
    for kk in NEAREST:
        out[kk] = sc.list_neighbors_brute(q, radii, md, k=kk)[0] if brute else sc.nearest_triangles(q, kk, radii, md)
    return out


def _assert_same_answers(got, want, what):
    assert (got["counts"] == want["counts"]).all(), (what, "counts", np.flatnonzero(got["counts"] != want["counts"])[:4])
    for key in ("listed", "plain") + NEAREST:
        assert nr.same(got[key], want[key]), (what, key, nr.first_difference(got[key], want[key]))


def _reference_answers(sd, q, radii, md, cache):
    full = nr.neighbors(sd, q, radii, md, dist2=cache)
    counts = np.diff(full[0]).astype(np.uint32)
    slots = _slots(counts)
    listed = nr.fill_slots(full, np.zeros(int(slots[-1]), nr.NEIGHBOR_DTYPE), offsets=slots)
    out = dict(counts=counts, slots=slots, listed=listed, plain=listed)
    for kk in NEAREST:
        out[kk] = nr.nearest(full, kk)
    return out


def _assert_neighbour_edges(k, q, ans):
    """What the run under the infinite radius must have reached."""
    rec, slots = ans["listed"], ans["slots"]
    assert not np.isnan(rec["dist2"]).any(), "a NaN never qualifies"
    if k == 62:
        tied = np.isposinf(rec["dist2"]) & (rec["prim_id"] != nr.NO_PRIM)
        assert tied.any(), "+inf dist2 qualifies under an infinite radius"
        for i in np.flatnonzero(np.isfinite(q).all(axis=1)):
            mine = rec[slots[i] : slots[i + 1]]
            ids = mine["prim_id"][np.isposinf(mine["dist2"])].astype(np.int64)
            assert (np.diff(ids) > 0).all(), (i, "records that tie at +inf are in prim_id order")
    if k == -70:
        assert ((rec["dist2"] > 0) & (rec["dist2"] < sr.FLT_MIN)).any(), "the sweep reaches denormal dist2 at 2^-70"


# ---- 1. neighbour parity at every k: cube and blob against the restatement ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SMALL)
def test_neighbour_parity_with_the_restatement(pkg, world, name, k):
    sd0 = world(name, 0)[0]
    sd, sc, q = world(name, k)
    cache = {}
    for label, radii, md in _bounds(sd0, k, len(q)):
        ref = _reference_answers(sd, q, radii, md, cache)
        brute = _device_answers(sc, q, radii, md, brute=True)
        tree = _device_answers(sc, q, radii, md, brute=False)
        _assert_same_answers(brute, ref, (name, k, label, "brute force against the restatement"))
        _assert_same_answers(tree, brute, (name, k, label, "tree search against brute force"))
        if label == "+inf":
            _assert_neighbour_edges(k, q, tree)
            if k == 0 and name != "cube":
                assert tree["counts"].max() > LIST_CAP, "the capped slots truncate"
        if label == "per query":
            dead = np.isnan(radii) | (radii < 0)
            zero = radii == 0  # (0.0 and -0.0)
            assert dead.sum() > 100 and not tree["counts"][dead].any()
            assert np.signbit(radii[zero]).any() and (~np.signbit(radii[zero])).any()
            if k in (-20, 0, 30):  # vertex queries (family 2) have dist2 == 0: both zeros admit them
                vertex = zero & (np.arange(len(q)) % 5 == 2) & (np.arange(len(q)) != 5) & (np.arange(len(q)) != 6)
                assert vertex.any() and (tree["counts"][vertex & np.signbit(radii)] > 0).all() and (tree["counts"][vertex & ~np.signbit(radii)] > 0).all()


# ---- 2. neighbour parity at every k: dodge and the dragon, tree against device brute force ----
@pytest.mark.parametrize("name,k", [(name, k) for name in LARGE for k in KS + EXTRA_KS.get(name, ())])
def test_neighbour_parity_on_the_large_scenes(pkg, world, name, k):
    sd0 = world(name, 0)[0]
    sd, sc, q = world(name, k)
    q = np.ascontiguousarray(q[:N_BRUTE])
    if k == 0:
        assert sc.num_subnodes() > 0, "dodge: the fixture with in-leaf accelerators; the dragon has them too"
    for label, radii, md in _bounds(sd0, k, len(q)):
        brute = _device_answers(sc, q, radii, md, brute=True)
        tree = _device_answers(sc, q, radii, md, brute=False)
        _assert_same_answers(tree, brute, (name, k, label, "tree search against brute force"))
        if label == "+inf":
            _assert_neighbour_edges(k, q, tree)
            assert (tree["counts"][np.isfinite(q).all(axis=1)] > 0).all()
        if label == "radius" and k == 0:
            assert tree["counts"].max() > LIST_CAP, "the capped slots truncate under the finite radius too"
            assert (tree["counts"] == 0).any()


# ---- 3. neighbour covariance on the device, and the work counters ----
def _neighbour_results(sc, q, r2):
    counts = sc.count_neighbors(q, max_dist2=r2)
    slots = _slots(counts)
    rec = sc.list_neighbors(q, max_dist2=r2, offsets=slots)[0] if slots[-1] else np.zeros(0, nr.NEIGHBOR_DTYPE)
    near = sc.nearest_triangles(q, 8)
    return (slots, rec), (np.arange(len(q) + 1, dtype=np.int64) * 8, near.reshape(-1))


def _neighbour_work(sc, q, r2):
    return sc.debug_neighbor_work(q, max_dist2=r2, k=0), sc.debug_neighbor_work(q, k=8)


@pytest.mark.parametrize("name", SMALL + LARGE)
def test_device_neighbours_are_covariant_inside_the_envelope(pkg, world, name):
    sd0, sc0, q0 = world(name, 0)
    r0 = _neighbour_results(sc0, q0, float(_r2(sd0, 0)))
    fin = np.isfinite(q0).all(axis=1)
    near = fin & (np.arange(N) % 5 != FAR)
    seen = {}
    for k in sorted(set(KS + EXTRA_KS.get(name, ())) - {0}):
        sd, sc, q = world(name, k)
        env = sr.in_envelope(sd, q)
        seen[k] = env
        if not env.any():
            continue
        rk = _neighbour_results(sc, q, float(_r2(sd0, k)))
        for what, a, b in (("radius lists", r0[0], rk[0]), ("eight nearest", r0[1], rk[1])):
            bad = np.flatnonzero(env & ~sr.covariant_neighbors(a, b, k))
            assert len(bad) == 0, (name, k, what, "not covariant inside the envelope", len(bad), int(bad[0]))
        sub0, subk = np.ascontiguousarray(q0[env]), np.ascontiguousarray(q[env])
        w0, wk = _neighbour_work(sc0, sub0, float(_r2(sd0, 0))), _neighbour_work(sc, subk, float(_r2(sd0, k)))
        print(f"{name}, 2^{k}: {int(env.sum())} of {int(fin.sum())} queries inside the envelope, all covariant; work {wk}")
        assert wk == w0, (name, k, "work counters", wk, w0)
    assert seen[30][near].all(), (name, "2^30 lies inside the envelope for the near families")
    low = -10 if name == "dodge" else -20
    assert seen[low][fin].all(), (name, low, "lies inside the envelope for every finite query")


# ---- 4. winding bytes at every k ----
def _assert_winding(got, want, what):
    (gw, gi), (ww, wi) = got, want
    gw, gi, ww, wi = (np.asarray(x).reshape(-1) for x in (gw, gi, ww, wi))
    assert gw.dtype == np.float32 and gi.dtype == np.bool_ and gw.shape == ww.shape and gi.shape == wi.shape, what
    bad = np.flatnonzero(~same_bits(gw, ww) | (gi != wi))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), gw[bad[0]], ww[bad[0]], gi[bad[0]], wi[bad[0]])


@pytest.mark.parametrize("name,k", [(name, k) for name in SMALL + LARGE for k in KS + EXTRA_KS.get(name, ())])
def test_winding_bytes_and_counters(pkg, world, name, k):
    sd0 = world(name, 0)[0]
    sd, sc, q = world(name, k)
    fin = np.isfinite(q).all(axis=1)
    tree_form, brute_form = sc.winding_numbers(q, beta=INF), sc.winding_numbers_brute(q)
    _assert_winding(tree_form, brute_form, (name, k, "the tree form at beta = +inf against the brute form"))
    w, inside = tree_form
    assert (~fin).sum() == 2 and (w[~fin].view(np.uint32) == 0).all() and not inside[~fin].any(), "non-finite points: +0 and 0"
    assert not inside[np.isnan(w)].any(), "a NaN is not inside"
    if k == 62:
        assert np.isnan(w[fin]).any(), "the sweep reaches NaN sums at 2^62"
    if k == 0:
        assert np.isfinite(w).all() and inside.any() and (~inside[fin]).any()
    # the stackless walk's counters are the restatement's, whatever the sums are
    qs = world.sign(name, k) if name in SMALL else world.few(name, k)
    tree = sc.debug_winding_tree()
    want = wr.walk(tree, wr.records(sd, tree), qs, 2.0, np.float32)[1]
    got = sc.debug_winding_work(qs, beta=2.0)
    assert got == want, (name, k, "counters at beta = 2", got, want)
    # the grid form against the list form
    for origin, spacing, dims in _grids(sd0, k):
        pts = pkg.sdf_grid_points(origin, spacing, dims)
        for beta in (2.0, INF):
            _assert_winding(sc.winding_grid(origin, spacing, dims, beta=beta), sc.winding_numbers(pts, beta=beta),
                            (name, k, dims, beta, "grid against the list form on sdf_grid_points"))


# ---- 5. winding numbers inside the envelope ----
def _winding_at_one(world, name):
    """The device's answers at scale 1 on the sign queries, once."""
    if name not in _w0:
        sd0, sc0, _ = world(name, 0)
        q0 = world.sign(name, 0)
        w, inside = sc0.winding_numbers(q0, beta=2.0)
        _w0[name] = (sd0, sc0, q0, sc0.debug_winding_tree(), w, inside)
    return _w0[name]


@pytest.mark.parametrize("name,k", [(name, k) for name in SMALL + LARGE for k in WINDING_INSIDE_KS if k >= INSIDE_LOW[name]])
def test_winding_inside_the_envelope(pkg, world, name, k):
    sd0, sc0, q0, tree0, w0, inside0 = _winding_at_one(world, name)
    sd, sc, _ = world(name, k)
    q = world.sign(name, k)
    tree = sc.debug_winding_tree()
    assert np.array_equal(tree["record_prims"], tree0["record_prims"]), (name, k, "the record order differs from scale 1")
    env = sr.in_winding_envelope(sd, q)
    assert env.all(), (name, k, "points outside the envelope", int((~env).sum()))
    assert sr.covariant_winding_tree(tree0, tree, k), (name, k, "the cluster tree is not the power-of-two image")
    work0, work = sc0.debug_winding_work(q0, beta=2.0), sc.debug_winding_work(q, beta=2.0)
    assert work == work0, (name, k, "counters", work, work0)
    recs = wr.records(sd, tree)
    w64, _ = wr.walk(tree, recs, q, 2.0, np.float64)
    w32, _ = wr.walk(tree, recs, q, 2.0, np.float32)
    w, inside = sc.winding_numbers(q, beta=2.0)
    scale = max(float(np.abs(w32.astype(np.float64) - w64).max()), FLOOR)
    err = float(np.abs(w.astype(np.float64) - w64).max())
    keep = np.abs(np.abs(w64) - 0.5) >= BAND
    print(f"{name}, 2^{k}: max |dev - walk64| {err:.3e}, max |walk32 - walk64| {scale:.3e}, ratio {err / scale:.2f}; {100.0 * (~keep).mean():.2f} % in "
          f"the band; device bits equal to the device's at scale 1 at {100.0 * same_bits(w, w0).mean():.1f} % of the points, to walk32 at "
          f"{100.0 * same_bits(w, w32).mean():.1f} %")
    assert scale <= 1e-3, "the float32 restatement itself is sound on these points (none on the surface)"
    assert err <= 4 * scale, (name, k, err, scale)
    assert (~keep).sum() <= 0.02 * len(q)
    assert inside[keep].any() and (~inside[keep]).any()
    assert (inside[keep] == inside0[keep]).all(), (name, k, int((inside != inside0)[keep].sum()))


# ---- 6. dipole-only points are IEEE ----
@pytest.mark.parametrize("name", SMALL + LARGE)
def test_dipole_only_points_have_the_restatements_bits(pkg, world, name):
    for k in (0,) + tuple(k for k in WINDING_INSIDE_KS if k >= INSIDE_LOW[name]):
        sd, sc, _ = world(name, k)
        q = world.far(name, k)
        assert sr.in_winding_envelope(sd, q).all(), (name, k)
        tree = sc.debug_winding_tree()
        w32, work = wr.walk(tree, wr.records(sd, tree), q, 2.0, np.float32)
        assert work[2] == 0 and work[0] == work[1] > 0 and (w32 != 0).all(), (name, k, "the far family is dipole-only", work)
        assert sc.debug_winding_work(q, beta=2.0) == work, (name, k)
        w = sc.winding_numbers(q, beta=2.0, want="w")
        bad = np.flatnonzero(w.view(np.uint32) != w32.view(np.uint32))
        assert len(bad) == 0, (name, k, "a dipole sum differs from the IEEE restatement", len(bad), int(bad[0]), w[bad[0]], w32[bad[0]])

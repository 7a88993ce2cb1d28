"""Query fuzz (run on the GPU box): every tree or grid search of include/cgrt.h against its brute form on random scenes, byte for byte,
and the brute forms against independent numpy / oracle computations on a subsample.  The header claims, per family, that the pruned
search returns the exhaustive one's bytes; the fixed scenes of the suite hold almost none of the inputs under which the two can differ
(exact ties in dist2 or t, duplicated triangles, meshes of 1, 2 or 9 triangles, many tiny meshes, leaves that cannot be split, scales
at the edge of an envelope).  This driver makes them.

Legs (exact: whole buffers, byte for byte; a NaN equals a NaN except in the frame records, whose NaNs the header canonicalises):
  A  closest points (host, tensor) == cgrt_closest_points_brute, max_dist2 in {+inf, 0, a dist2 the brute form returned}
  B  crossings: counts, first k in {1, 2, 7, 33} with and without counts, full CSR lists == cgrt_list_crossings_brute
  C  neighbours: counts, k nearest with and without counts, full lists, scalar and per-query radii == cgrt_list_neighbors_brute; N1
  D  signed distance (list, host, 5 x 4 x 3 grid) == the composition of the brute closest points and the brute crossing counts
  E  winding numbers at beta = +inf (host, tensor, grid) == cgrt_winding_numbers_brute
  F  point sets: grid counts, lists, k nearest, frames, knn frames, Poisson-disk sets == their brute forms, any cell size
Reference legs (scenes of at most 300 triangles / data points, the first 128 queries): the device's brute records against
tests/closest_ref.py, neighbors_ref.py, crossings_ref.py (the oracle), point_neighbors_ref.py, point_frames_ref.py byte for byte, and
inside the envelopes of tests/scale_ref.py against float64: the header's 5.66 * 2^-24 * max(1, |p|inf, S) for distances and
memberships, and the winding numbers' largest error (reported; tests/test_fuzz_queries_gpu.py holds it).

Iteration `it` of seed `seed0` draws everything from np.random.default_rng([seed0, it, tag]): a failure reproduces from (seed,
iteration, leg).  run() returns statistics and judges nothing; the command line does:
    python tools/fuzz_queries.py [seconds] [seed] [leg ...]        exit status 1 on any mismatch
tests/test_fuzz_queries_gpu.py calls run() with fixed iteration counts over tests/fuzz_query_seeds.txt."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import __graft_entry__ as e  # noqa: E402

pkg = e.load_package()
import closest_ref as cr  # noqa: E402
import crossings_ref as xr  # noqa: E402
import fuzz_scenes  # noqa: E402
import neighbors_ref as nr  # noqa: E402
import point_frames_ref as fref  # noqa: E402
import point_neighbors_ref as pnr  # noqa: E402
import poisson_ref  # noqa: E402
import scale_ref  # noqa: E402

F32 = np.float32
INF = float("inf")
NO_PRIM = 0xFFFFFFFF
ALL = ("A", "B", "C", "D", "E", "F")
KINDS = ("soup", "lattice", "stand-in", "sliver", "holes")
TRI_COUNTS = (1, 2, 9, 65, 513, 1500, 6000)  # 9, 65, 513: one, two, three levels of the winding cluster tree; 1, 2: a tree of one leaf
SCALES = (0, 0, 0, -20, -8, 7, 19, 30, 37)  # fuzz_parity's
SIZES = (1, 63, 64, 65, 257, 1000)
SLOT_K = (1, 2, 7, 33)
POINT_K = (1, 2, 8, 33)
CLOUD_KINDS = ("lattice", "clustered", "uniform", "holes")
CLOUD_SIZES = (1, 7, 300, 3000)
CLOUD_SCALES = (0, -40, -8, 8, 40)
CELL_STEPS = tuple(range(-4, 5))
FULL_LIST_CAP = 1024  # a slot is insertion-sorted: a full list costs count^2 per query
REF_TRIS = 300  # reference legs: scenes (clouds) of at most this many triangles (points) ...
REF_QUERIES = 128  # ... and the first this many queries
K_CLOSEST = 5.66  # include/cgrt.h "Closest-point queries": the accuracy bound's factor on well-shaped meshes (tests/test_neighbors_cpu.py K)
# How far the DEFINITION (tests/closest_ref.py, float32) is from the float64 distance on this fuzz's scenes, in units of that bound: the
# largest value over the reference subsamples of the committed seeds, measured on the CPU and held to its measurement by
# tests/test_fuzz_queries_cpu.py::test_reference_bounds_hold_on_the_cpu.  5.66 is a measurement on meshes of moderate aspect; on a sliver
# whose short edge is about an ulp of its coordinates (aspect 1e7: seed 6606, iteration 3, query 126, a sliver scene at 2^30) the
# interior region's 1 / ((va + vb) + vc) cancels and the defined point lies 0.017 extents from the nearest one.  The device's brute form
# returns the restatement's bytes, so it is held to the same figure with no margin.
CLOSEST_F32_RATIO = 54400.0
TAG_PLAN, TAG_SCENE, TAG_POINTS, TAG_RAYS, TAG_CLOUD, TAG_LEG = 0, 1, 2, 3, 4, 16
_ERR = dict(all="ignore")


def _rng(seed0, it, tag):
    return np.random.default_rng([int(seed0), int(it), int(tag)])


def _plan(seed0):
    """What is stratified rather than drawn anew per iteration, so that few iterations see every scene kind, triangle count, cloud
    kind, cloud size and cell step: per seed one permutation of each; iteration `it` takes entry it mod the length."""
    g = np.random.default_rng([int(seed0), TAG_PLAN])
    return dict(kind=g.permutation(len(KINDS)), tris=g.permutation(len(TRI_COUNTS)), ckind=g.permutation(len(CLOUD_KINDS)),
                csize=g.permutation(len(CLOUD_SIZES)), cell=g.permutation(len(CELL_STEPS)))


# ---- generators: numpy only, deterministic in (seed0, it) ----
class FuzzScene:
    def __init__(self, kind, base_kind, tris, k, base):
        self.kind, self.base_kind, self.tris, self.k = kind, base_kind, tris, k
        self.base = base  # at scale 1: the queries are made here and scaled with the scene, exactly
        self.sd = scale_ref.scaled(base, k)

    def describe(self):
        return f"kind {self.kind}" + (f" ({self.base_kind})" if self.kind == "holes" else "") + f" scale 2^{self.k} tris {self.sd.ntris}"


def _base_scene(kind, T, g):
    rs = np.random.RandomState(int(g.integers(1, 1 << 31)))  # the shared generators take the legacy interface
    if kind == "soup":
        tiny = bool(g.integers(0, 2))  # half the soups are trees of many tiny meshes
        return fuzz_scenes.soup(rs, max_tris=T, sizes=(1, 2, 5) if tiny else fuzz_scenes.SOUP_SIZES)
    if kind == "lattice":
        return fuzz_scenes.lattice(g, T)
    if kind == "sliver":
        import test_adversarial_gpu as adv

        return adv._sliver_scene(pkg, rs, ntris=T, with_dragon=False)
    make = (pkg.scenes.make_dragon, pkg.scenes.make_dragon_irregular, pkg.scenes.make_blob)[int(g.integers(0, 3))]
    return make(int(g.integers(3000, 9001)), seed=int(g.integers(1, 1 << 30)))


def make_scene(seed0, it):
    """The scene of iteration `it`: its kind and triangle count from the seed's plan, the rest drawn."""
    plan, g = _plan(seed0), _rng(seed0, it, TAG_SCENE)
    kind = KINDS[int(plan["kind"][it % len(KINDS)])]
    T = TRI_COUNTS[int(plan["tris"][it % len(TRI_COUNTS)])]
    k = int(g.choice(SCALES))
    base_kind = kind if kind != "holes" else KINDS[int(g.integers(0, 4))]
    sd = _base_scene(base_kind, T, g)
    if kind == "holes":
        sd = fuzz_scenes.punched(sd, g)
    return FuzzScene(kind, base_kind, 0 if base_kind == "stand-in" else T, k, sd)


def _unit(g, n):
    d = g.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def make_points(fs, seed0, it):
    """(n, 3) float32 query points of iteration `it`, n from SIZES: closest_ref.mixed_queries of the scale-1 scene; three rows in ten
    replaced by lattice points and cell centres (on lattice scenes: equidistant from many triangles), points beyond 2^40 scene sizes
    and non-finite points; all scaled with the scene."""
    g = _rng(seed0, it, TAG_POINTS)
    n = int(g.choice(SIZES))
    with np.errstate(**_ERR):
        P = cr.mixed_queries(fs.base, n, int(g.integers(1, 1 << 30)))
    for i in np.flatnonzero(g.random(n) < 0.3):
        u = g.random()
        if u < 0.1:
            P[i] = (_unit(g, 1)[0] * 2.0 ** 41).astype(F32)
        elif u < 0.2:
            P[i, g.integers(0, 3)] = (np.nan, np.inf, -np.inf)[int(g.integers(0, 3))]
        elif fs.base_kind == "lattice" or u < 0.4:
            P[i] = g.integers(-10, 11, 3) * 0.125  # multiples of 1/4: lattice points; odd multiples of 1/8: cell centres
    return scale_ref.scaled_points(P, fs.k)


def make_rays(fs, seed0, it):
    """(n, 7) float32 rays of iteration `it`, n from SIZES: the families of crossings_ref that need no oracle, interleaved, and
    axis-parallel rays through lattice points (vertices, off lattice scenes); a third of the aimed rays end exactly at their target
    (t = 1); where n allows the two non-finite rays, an origin beyond 2^40, a direction below 2^-40 and a NaN t.  Made on the scale-1
    scene, origins and t scaled with it."""
    g = _rng(seed0, it, TAG_RAYS)
    n = int(g.choice(SIZES))
    m, s, b = n // 6 + 1, int(g.integers(1, 1 << 30)), fs.base
    with np.errstate(**_ERR):
        aimed = xr.edge_and_vertex_rays(b, m, s + 2)
        aimed[2::3, 6] = 1.0
        pos = xr.positions(b)
        axis, sign = g.integers(0, 3, m), g.choice([-1.0, 1.0], m)
        through = pos[g.integers(0, len(pos), m)] if fs.base_kind != "lattice" else (g.integers(-4, 5, (m, 3)) * 0.25).astype(F32)
        d = np.zeros((m, 3), F32)
        d[np.arange(m), axis] = sign * g.choice([0.5, 1.0, 2.0], m)
        d[np.arange(m), (axis + 1) % 3] = g.choice([0.0, -0.0], m)
        lines = xr._rays(through - d * g.integers(0, 5, (m, 1)).astype(F32), d)
        fams = [xr.random_rays(b, m, s), xr.vertex_origin_rays(b, m, s + 1), aimed, xr.t_zero_rays(b, m, s + 3),
                xr.zero_component_rays(b, m, s + 4), lines]
        R = np.stack(fams, axis=1).reshape(-1, 7)[:n].copy()
        if n >= 63:
            R[5], R[40] = xr.nan_inf_rays()
            R[7, 0:3] = (_unit(g, 1)[0] * 2.0 ** 41).astype(F32)
            R[9, 3:6] = (_unit(g, 1)[0] * 2.0 ** -45).astype(F32)
            R[11, 6] = np.nan
            R[13, 3:6] = (_unit(g, 1)[0] * 2.0 ** 41).astype(F32)
    return scale_ref.scaled_rays(R, fs.k)


def irregular_rays(R):
    """(n,) bool: outside the box test's envelope (walk_exact.h make_raypre: non-finite or beyond 2^40, no component of the direction of
    2^-40 or more, a NaN t): such a ray tests every triangle itself."""
    with np.errstate(**_ERR):
        fin = (np.abs(R[:, 0:6]) <= 2.0 ** 40).all(axis=1)
        return ~fin | ~(np.abs(R[:, 3:6]).max(axis=1) >= 2.0 ** -40) | np.isnan(R[:, 6])


class FuzzCloud:
    pass


def make_cloud(seed0, it):
    """The point set, queries, radii and cell of iteration `it` of leg F.  Lattice clouds have coordinates that are multiples of 1/8
    with one row in ten a copy of an earlier one, and radii that are exact squared lattice distances: ties in d2 and at the bound."""
    plan, g = _plan(seed0), _rng(seed0, it, TAG_CLOUD)
    c = FuzzCloud()
    c.kind = CLOUD_KINDS[int(plan["ckind"][it % len(CLOUD_KINDS)])]
    m = c.m = CLOUD_SIZES[int(plan["csize"][(it // 2) % len(CLOUD_SIZES)])]
    c.k = int(g.choice(CLOUD_SCALES))
    c.step = CELL_STEPS[int(plan["cell"][it % len(CELL_STEPS)])]
    shape = c.kind if c.kind != "holes" else ("lattice", "uniform")[int(g.integers(0, 2))]
    if shape == "lattice":
        data = g.integers(0, 9, (m, 3)) * 0.125
        for i in np.flatnonzero(g.random(m) < 0.1):
            data[i] = data[g.integers(0, i + 1)]
    elif shape == "clustered":
        centres = g.random((12, 3))
        data = centres[g.integers(0, 12, m)] + 0.01 * g.normal(size=(m, 3))
    else:
        data = g.random((m, 3))
    data = data.astype(F32)
    if c.kind == "holes":
        for i in g.integers(0, m, 1 + m // 50):
            data[i, g.integers(0, 3)] = (np.nan, np.inf, -np.inf)[int(g.integers(0, 3))]
    n = c.n = int(g.choice(SIZES))
    pts = g.random((n, 3))
    own = min(n, m)
    pts[:own] = data[:own]  # query i is data point i: skip_same_index means something
    for i in range(own, n):
        u = g.random()
        if u < 0.4:
            pts[i] = data[g.integers(0, m)] + (0.0 if u < 0.1 else 0.02 * g.normal(size=3))
        elif u < 0.6 and shape == "lattice":
            pts[i] = g.integers(0, 17, 3) * 0.0625  # lattice points and cell centres
        elif u < 0.65:
            pts[i, g.integers(0, 3)] = (np.nan, np.inf)[int(g.integers(0, 2))]
    pts = pts.astype(F32)
    with np.errstate(**_ERR):
        if shape == "lattice":
            r2 = float(g.choice([1, 2, 3, 4, 8])) / 64.0
        else:
            d2 = pnr.d2_matrix(pts[: min(n, 64)], data[: min(m, 512)]).reshape(-1)
            d2 = d2[np.isfinite(d2) & (d2 > 0)]
            r2 = float(np.sort(d2)[min(len(d2) - 1, int(len(d2) * g.uniform(0.002, 0.05)))]) if len(d2) else 0.01
    rad = (F32(r2) * g.choice([0.25, 1.0, 1.0, 4.0], n)).astype(F32)
    sp = g.random(n)
    rad[sp < 0.03], rad[(sp >= 0.03) & (sp < 0.06)], rad[(sp >= 0.06) & (sp < 0.09)] = np.nan, -1.0, 0.0
    if m <= REF_TRIS:
        rad[(sp >= 0.09) & (sp < 0.12)] = np.inf
    with np.errstate(**_ERR):
        c.data, c.points = np.ldexp(data, c.k).astype(F32), np.ldexp(pts, c.k).astype(F32)
        c.r2 = float(np.ldexp(F32(r2), 2 * c.k))
        c.radius2 = np.ldexp(rad, 2 * c.k).astype(F32)
        c.cell = float(np.ldexp(np.sqrt(r2), c.k + c.step))
    c.orient = g.normal(size=(n, 3)).astype(F32) if g.integers(0, 2) else None
    c.skip = bool(g.integers(0, 2))
    c.frame_k = [int(x) for x in g.choice(POINT_K, 2, replace=False)]
    c.poisson = dict(min_dist2=float(np.ldexp(F32(r2) * F32(g.choice([0.25, 1.0, 4.0])), 2 * c.k)), seed=int(g.integers(0, 1 << 31)),
                     priority=g.integers(0, max(2, m // 4), m).astype(np.uint32) if g.integers(0, 2) else None)
    return c


# ---- comparing ----
def same(a, b, strict=False):
    """Whole buffers, byte for byte; unless `strict`, float32 words that are NaN on both sides count as equal (fuzz_parity.same)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.tobytes() == b.tobytes():
        return True
    if strict:
        return False
    if a.dtype.names:
        return all(same(a[f], b[f]) for f in a.dtype.names)
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return False


def first_difference(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shapes {a.shape} {b.shape}, types {a.dtype} {b.dtype}"
    a, b = a.reshape(-1), b.reshape(-1)
    for i in range(len(a)):
        if not same(a[i : i + 1], b[i : i + 1]):
            return f"record {i}: {a[i]} != {b[i]}"
    return "equal up to NaN payloads"


class Run:
    """The statistics of a run and the context a mismatch is printed with."""

    def __init__(self, seed0, verbose):
        self.seed0, self.verbose, self.it, self.leg, self.what = seed0, verbose, 0, "", ""
        self.stats = dict(iterations=0, comparisons=0, mismatches=0, queries=0)

    def add(self, key, v=1):
        self.stats[key] = self.stats.get(key, 0) + int(v)

    def top(self, key, v):
        self.stats[key] = max(self.stats.get(key, 0.0), float(v))

    def check(self, name, got, want, strict=False):
        self.stats["comparisons"] += 1
        if same(got, want, strict):
            return True
        self.fail(name, first_difference(got, want))
        return False

    def fail(self, name, detail):
        self.stats["mismatches"] += 1
        self.add("mismatches_" + self.leg)
        print(f"MISMATCH: seed {self.seed0} iteration {self.it} leg {self.leg} {self.what}: {name}: {detail}", flush=True)


def _np(t):
    return t.detach().cpu().numpy()


def _records(t, dtype):
    """A float32 tensor whose last axis is one record, as a numpy array of `dtype` records."""
    a = np.ascontiguousarray(_np(t))
    return a.view(dtype).reshape(a.shape[:-1])


def _ties(rec, key, ident):
    """Slots ((n, k) records) that hold two consecutive real records with equal keys: the tie rule decided their order."""
    if rec.ndim != 2 or rec.shape[1] < 2:
        return 0
    return int(((rec[key][:, 1:] == rec[key][:, :-1]) & (rec[ident][:, 1:] != NO_PRIM)).any(axis=1).sum())


def _csr_ties(off, rec, key):
    eq = np.flatnonzero(rec[key][1:] == rec[key][:-1]) + 1  # record j equals record j - 1 ...
    return int(len(np.unique(np.searchsorted(off, eq[~np.isin(eq, off)], side="right"))))  # ... and both belong to one query


def _slot_stats(R, fam, rec, counts, k, key, ident):
    R.add(f"{fam}_tie_slots", _ties(rec, key, ident))
    R.add(f"{fam}_overfull_slots", (counts > k).sum())
    R.add(f"{fam}_short_slots", (counts < k).sum())
    R.add(f"{fam}_exact_slots", (counts == k).sum())


def _a_dist2(g, d2):
    """One of the finite values of d2 (or 1): a bound some record meets exactly."""
    v = d2[np.isfinite(d2)]
    return float(v[g.integers(0, len(v))]) if len(v) else 1.0


def _torch():
    import torch

    return torch


def _dev(a, dtype=None):
    t = _torch().from_numpy(np.ascontiguousarray(a).copy())
    return (t if dtype is None else t.to(dtype)).cuda()


def _scene_stats(R, fs, sc):
    bi = sc.build_info()
    R.add("kind_" + fs.kind)
    R.add(f"tris_{fs.tris}")
    R.add("scenes_wild_leaves", bi["wild_leaves"] > 0)
    R.add("scenes_non_finite", not bi["geometry_finite"])
    R.add("scenes_tree_search", bi["wild_leaves"] == 0 and bi["geometry_finite"])
    if fs.kind == "holes":
        R.stats["comparisons"] += 1
        if bi["geometry_finite"]:
            R.fail("build_info", "a scene with a NaN and an infinite vertex reports finite geometry: no brute fallback")
    return bi


# ---- leg A: closest points ----
def leg_closest(R, fs, sc, g):
    P = make_points(fs, R.seed0, R.it)
    dP = _dev(P)
    R.add("queries", len(P))
    ref_inf = sc.closest_points_brute(P)
    for md in (INF, 0.0, _a_dist2(g, ref_inf["dist2"])):
        want = ref_inf if md == INF else sc.closest_points_brute(P, md)
        R.check(f"closest_points(max_dist2={md})", sc.closest_points(P, md), want)
        R.check(f"closest_points_tensor(max_dist2={md})", _records(sc.closest_points_tensor(dP, md)["out"], pkg.CLOSEST_DTYPE), want)
        R.add("closest_hits", (want["prim_id"] != NO_PRIM).sum())
        R.add("closest_misses", (want["prim_id"] == NO_PRIM).sum())
    if fs.sd.ntris <= REF_TRIS:
        ref_closest(R, fs, P[:REF_QUERIES], ref_inf[:REF_QUERIES])


def _envelope(predicate, sd, P, **kw):
    """scale_ref's envelope predicate; nobody is inside on a scene that has no finite triangle of non-zero area to measure."""
    try:
        with np.errstate(**_ERR):
            return predicate(sd, P, **kw)
    except ValueError:  # (the smallest of no areas / edges)
        return np.zeros(len(P), bool)


def closest_bound(sd, P):
    """(n,) float64: 5.66 * 2^-24 * max(1, |p|inf, S), the header's accuracy bound on a distance."""
    with np.errstate(**_ERR):
        return K_CLOSEST * 2.0 ** -24 * np.maximum(np.maximum(1.0, np.abs(np.asarray(P, np.float64)).max(axis=1)), cr.scene_scale(sd))


def closest_error(sd, P, rec):
    """(error over bound (n,), which queries count): |sqrt(dist2) - float64 distance| over the header's bound, for the queries inside
    the envelope that found a triangle."""
    with np.errstate(**_ERR):
        d64 = cr.dist64(sd, P)
        d64 = np.where(np.isnan(d64), np.inf, d64).min(axis=1)
        ok = _envelope(scale_ref.in_envelope, sd, P) & (rec["prim_id"] != NO_PRIM) & np.isfinite(d64)
        ratio = np.abs(np.sqrt(rec["dist2"].astype(np.float64)) - d64) / closest_bound(sd, P)
    return np.where(ok, ratio, 0.0), ok


def ref_closest(R, fs, P, dev):
    with np.errstate(**_ERR):
        R.check("closest_points_brute against closest_ref.brute", dev, cr.brute(fs.sd, P).astype(pkg.CLOSEST_DTYPE))
    ratio, ok = closest_error(fs.sd, P, dev)
    R.add("ref_closest_bounded", ok.sum())
    R.top("ref_closest_max_ratio", ratio.max() if len(ratio) else 0.0)
    R.stats["comparisons"] += 1
    if (ratio > CLOSEST_F32_RATIO).any():
        i = int(ratio.argmax())
        R.fail("closest accuracy", f"query {i} {P[i]}: {ratio[i]:.3f} times {K_CLOSEST} * 2^-24 * max(1, |p|inf, S), above {CLOSEST_F32_RATIO}")


# ---- legs B and C: the slot families ----
def _slot_leg(R, fam, n, k_list, brute, first_host, first_tensor, count_forms, full_forms, key, ident, must_list):
    """The comparisons every slot family makes.  brute(k) -> (records (n, k), counts) and brute(0) -> (offsets, records); first_host(k,
    want_counts) -> (records, counts or None); first_tensor(k, want_counts) -> the same, as numpy; count_forms / full_forms: name ->
    callable.  Returns the brute counts."""
    rec1, counts = brute(1)
    for name, f in count_forms.items():
        R.check(name, np.asarray(f()).astype(np.uint32), counts)
    for k in k_list:
        want, wc = (rec1, counts) if k == 1 else brute(k)
        R.check(f"{fam} brute counts(k={k})", wc, counts)
        _slot_stats(R, fam, want, counts, k, key, ident)
        for with_counts in (True, False):
            got, gc = first_host(k, with_counts)
            R.check(f"{fam} first {k} host records (counts={with_counts})", got, want)
            if with_counts:
                R.check(f"{fam} first {k} host counts", gc, counts)
            tt = first_tensor(k, with_counts)
            if tt is not None:
                R.check(f"{fam} first {k} tensor records (counts={with_counts})", tt[0], want)
                if tt[1] is not None:
                    R.check(f"{fam} first {k} tensor counts", tt[1].astype(np.uint32), counts)
    if int(counts.max(initial=0)) <= FULL_LIST_CAP:
        off, rec = brute(0)
        R.add(f"{fam}_full_lists")
        R.add(f"{fam}_tie_lists", _csr_ties(off, rec, key))
        for name, f in full_forms.items():
            o, r = f()
            R.check(name + " offsets", np.asarray(o, np.int64), off)
            R.check(name + " records", r, rec)
    else:
        R.add(f"{fam}_full_lists_skipped")
        R.add(f"{fam}_full_lists_skipped_where_required", must_list)
    return rec1, counts


def leg_crossings(R, fs, sc, g):
    rays = make_rays(fs, R.seed0, R.it)
    d = _dev(rays)
    n = len(rays)
    R.add("queries", n)
    R.add("rays_outside_box_envelope", irregular_rays(rays).sum())
    dt = pkg.CROSSING_DTYPE

    def tensor_first(k, with_counts):
        if not with_counts:
            return None  # (first_crossings_tensor always counts; the shrinking bound is the host form's)
        rec, cnt = sc.first_crossings_tensor(d, k)
        return _records(rec, dt), _np(cnt)

    def tensor_full():
        off, rec = sc.list_crossings_tensor(d)
        return _np(off), _records(rec, dt).reshape(-1)

    rec1, counts = _slot_leg(
        R, "crossings", n, SLOT_K, lambda k: sc.list_crossings_brute(rays, k=k), lambda k, c: sc.first_crossings(rays, k, want_counts=c),
        tensor_first, {"count_crossings": lambda: sc.count_crossings(rays), "count_crossings_tensor": lambda: _np(sc.count_crossings_tensor(d))},
        {"list_crossings": lambda: sc.list_crossings(rays), "list_crossings_tensor": tensor_full}, "t", "prim_id", abs(fs.k) <= 19)
    R.add("crossings_total", counts.sum())
    if fs.sd.ntris <= REF_TRIS and int(counts[:REF_QUERIES].max(initial=0)) <= FULL_LIST_CAP:
        r = rays[:REF_QUERIES]
        c, off, rec = xr.reference(_oracle(), fs.sd, r)
        doff, drec = sc.list_crossings_brute(r)
        R.add("ref_crossings_rays", len(r))
        R.check("list_crossings_brute against the oracle: counts", np.diff(doff).astype(np.uint32), c)
        R.check("list_crossings_brute against the oracle: records", drec, rec.astype(dt))


def radii(g, n, d2near):
    """(n,) float32 per-query squared radii: nearest-triangle dist2 values of the list times 1, 4 or 16, and NaN, negative, 0 and +inf
    entries."""
    v = d2near[np.isfinite(d2near)]
    with np.errstate(**_ERR):
        r = ((v[g.integers(0, len(v), n)] if len(v) else np.ones(n, F32)) * g.choice([1.0, 4.0, 16.0], n)).astype(F32)
    u = g.random(n)
    r[u < 0.04], r[(u >= 0.04) & (u < 0.08)], r[(u >= 0.08) & (u < 0.12)], r[(u >= 0.12) & (u < 0.15)] = np.nan, -1.0, 0.0, np.inf
    return r


def leg_neighbors(R, fs, sc, g):
    P = make_points(fs, R.seed0, R.it)
    dP = _dev(P)
    n = len(P)
    R.add("queries", n)
    dt = pkg.NEIGHBOR_DTYPE
    near = sc.closest_points_brute(P)["dist2"]
    with np.errstate(**_ERR):
        md = float(F32(_a_dist2(g, near)) * F32(g.choice([1.0, 4.0])))
    md = md if np.isfinite(md) else INF
    rad = radii(g, n, near)
    for mode, r2, kw in (("scalar", None, dict(max_dist2=md)), ("per-query", rad, dict(radius2=rad))):
        tkw = dict(max_dist2=md) if r2 is None else dict(radius2=_dev(rad))

        def tensor_first(k, with_counts):
            got = sc.nearest_triangles_tensor(dP, k, want_counts=with_counts, **tkw)
            return (_records(got[0], dt), _np(got[1])) if with_counts else (_records(got, dt), None)

        def host_first(k, with_counts):
            got = sc.nearest_triangles(P, k, want_counts=with_counts, **kw)
            return got if with_counts else (got, None)

        def tensor_full():
            off, rec = sc.list_neighbors_tensor(dP, **tkw)
            return _np(off), _records(rec, dt).reshape(-1)

        rec1, counts = _slot_leg(
            R, "neighbors", n, SLOT_K, lambda k: sc.list_neighbors_brute(P, k=k, **kw), host_first, tensor_first,
            {f"count_neighbors ({mode})": lambda: sc.count_neighbors(P, **kw),
             f"count_neighbors_tensor ({mode})": lambda: _np(sc.count_neighbors_tensor(dP, **tkw))},
            {f"list_neighbors ({mode})": lambda: sc.list_neighbors(P, **kw), f"list_neighbors_tensor ({mode})": tensor_full},
            "dist2", "prim_id", False)
        R.add("neighbors_total", counts.sum())
        if r2 is None:  # N1: the k = 1 records are {dist2, prim_id} of the closest points
            c = sc.closest_points(P, md)
            n1 = np.zeros(n, dt)
            n1["dist2"], n1["prim_id"] = c["dist2"], c["prim_id"]
            R.check("N1: nearest_triangles(k=1) against closest_points", rec1.reshape(-1), n1)
        if fs.sd.ntris <= REF_TRIS:
            ref_neighbors(R, fs, sc, P[:REF_QUERIES], None if r2 is None else rad[:REF_QUERIES], md)


def ref_neighbors(R, fs, sc, P, rad, md):
    kw = dict(max_dist2=md) if rad is None else dict(radius2=rad)
    doff, drec = sc.list_neighbors_brute(P, **kw)
    with np.errstate(**_ERR):
        off, rec = nr.neighbors(fs.sd, P, **kw)
        R.check("list_neighbors_brute against neighbors_ref: offsets", doff, off)
        R.check("list_neighbors_brute against neighbors_ref: records", drec, rec.astype(pkg.NEIGHBOR_DTYPE))
        # membership against float64, for every pair farther from the radius than the accuracy band (CLOSEST_F32_RATIO header bounds)
        r2 = nr.bounds(len(P), rad, md).astype(np.float64)
        d64 = cr.dist64(fs.sd, P)
        member = np.zeros(d64.shape, bool)
        member[np.repeat(np.arange(len(P)), np.diff(doff)), drec["prim_id"].astype(np.int64)] = True
        live = _envelope(scale_ref.in_envelope, fs.sd, P) & (r2 >= 0) & np.isfinite(r2)
        clear = live[:, None] & np.isfinite(d64) & (np.abs(d64 - np.sqrt(np.where(live, r2, 0.0))[:, None]) > CLOSEST_F32_RATIO * closest_bound(fs.sd, P)[:, None])
        bad = clear & (member != (d64 <= np.sqrt(np.where(live, r2, 0.0))[:, None]))
    R.add("ref_neighbors_pairs", clear.sum())
    R.stats["comparisons"] += 1
    if bad.any():
        q, t = np.argwhere(bad)[0]
        R.fail("neighbour membership against float64", f"query {q} {P[q]} triangle {t}: float64 distance {d64[q, t]}, radius {np.sqrt(r2[q])}")


_ORC = []


def _oracle():
    if not _ORC:
        o = e.load_oracle()
        if not os.path.exists(o.LIB):
            o.build()
        _ORC.append(o)
    return _ORC[0]


# ---- leg D: signed distance ----
def sdf_from_brute(sc, P, md):
    """test_sdf_gpu._composition fed from the brute entries, under the rule of tests/sdf_ref.py: (sdf (n,) float32, inside (n,) bool)."""
    P = np.ascontiguousarray(P, F32).reshape(-1, 3)
    votes = np.zeros(len(P), np.int64)
    for d in pkg.INSIDE_DIRECTIONS:
        rays = np.zeros((len(P), 7), F32)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6] = P, np.asarray(d, F32), np.inf
        votes += sc.list_crossings_brute(rays, k=1)[1].astype(np.int64) & 1
    inside = votes > len(pkg.INSIDE_DIRECTIONS) // 2
    with np.errstate(**_ERR):
        s = np.sqrt(sc.closest_points_brute(P, md)["dist2"])
    assert s.dtype == np.float32
    sdf = np.where(inside, -s, s)
    finite = np.isfinite(P).all(axis=1)
    sdf[~finite], inside[~finite] = np.inf, False
    return sdf, inside


def _grid(fs, g):
    """(origin, spacing) of a grid about the scene: fractions of its box, a zero or negative spacing now and then; scaled with it."""
    with np.errstate(**_ERR):
        lo, hi = cr.scene_box(fs.base)
    ext = np.maximum(np.nan_to_num(hi - lo), 1e-3)
    origin = (np.nan_to_num(lo) + ext * g.uniform(-0.2, 0.5, 3)).astype(F32)
    spacing = (ext * g.uniform(0.05, 0.3, 3) * g.choice([1.0, 1.0, 1.0, -1.0, 0.0], 3)).astype(F32)
    return tuple(float(x) for x in np.ldexp(origin, fs.k)), tuple(float(x) for x in np.ldexp(spacing, fs.k))


GRID_DIMS = (5, 4, 3)


def leg_sdf(R, fs, sc, g):
    P = make_points(fs, R.seed0, R.it)
    dP = _dev(P)
    R.add("queries", len(P))
    near = sc.closest_points_brute(P)["dist2"]
    for md in (INF, _a_dist2(g, near)):
        ws, wi = sdf_from_brute(sc, P, md)
        s, i = sc.sdf_tensor(dP, max_dist2=md)
        R.check(f"sdf_tensor sdf (max_dist2={md})", _np(s), ws)
        R.check(f"sdf_tensor inside (max_dist2={md})", _np(i), wi)
        s, i = sc.sdf(P, max_dist2=md)
        R.check(f"sdf host sdf (max_dist2={md})", s, ws)
        R.check(f"sdf host inside (max_dist2={md})", i, wi)
        R.add("sdf_inside", wi.sum())
        R.add("sdf_outside", (~wi).sum())
    origin, spacing = _grid(fs, g)
    gp = pkg.sdf_grid_points(origin, spacing, GRID_DIMS)
    ls, li = sc.sdf_tensor(_dev(gp))
    gs, gi = sc.sdf_grid_tensor(origin, spacing, GRID_DIMS)
    R.check("sdf_grid_tensor sdf against the list form", _np(gs).reshape(-1), _np(ls))
    R.check("sdf_grid_tensor inside against the list form", _np(gi).reshape(-1), _np(li))
    ws, wi = sdf_from_brute(sc, gp, INF)
    R.check("sdf on the grid points against the brute composition", _np(ls), ws)
    R.check("inside on the grid points against the brute composition", _np(li), wi)


# ---- leg E: winding numbers ----
def leg_winding(R, fs, sc, g):
    P = make_points(fs, R.seed0, R.it)
    dP = _dev(P)
    R.add("queries", len(P))
    ww, wi = sc.winding_numbers_brute(P)
    w, i = sc.winding_numbers(P, beta=INF)
    R.check("winding_numbers(beta=inf) w", w, ww)
    R.check("winding_numbers(beta=inf) inside", i, wi)
    w, i = sc.winding_numbers_tensor(dP, beta=INF)
    R.check("winding_numbers_tensor(beta=inf) w", _np(w), ww)
    R.check("winding_numbers_tensor(beta=inf) inside", _np(i), wi)
    R.add("winding_inside", wi.sum())
    R.add("winding_nan", np.isnan(ww).sum())
    origin, spacing = _grid(fs, g)
    gp = pkg.sdf_grid_points(origin, spacing, GRID_DIMS)
    gw, gi = sc.winding_numbers_brute(gp)
    w, i = sc.winding_grid_tensor(origin, spacing, GRID_DIMS, beta=INF)
    R.check("winding_grid_tensor(beta=inf) w", _np(w).reshape(-1), gw)
    R.check("winding_grid_tensor(beta=inf) inside", _np(i).reshape(-1), gi)
    if fs.sd.ntris <= REF_TRIS:
        err, ok, off = winding_error(fs.sd, P[:REF_QUERIES], ww[:REF_QUERIES])
        R.add("ref_winding_bounded", ok.sum())
        R.add("ref_winding_bounded_off_surface", off.sum())
        R.top("ref_winding_max_err", err.max(initial=0.0))
        R.top("ref_winding_off_surface_max_err", err[off].max(initial=0.0))


def surface_dist64(sd, P):
    """(n,) float64 distance from every point to the nearest triangle: closest_ref.dist64, and for the pairs it cannot answer (a
    triangle of zero area: 0 / 0 in the interior region) the distance to the triangle's three edges."""
    with np.errstate(**_ERR):
        p = np.asarray(P, np.float64).reshape(-1, 1, 3)
        d = cr.dist64(sd, P)
        v = cr.tri_verts(sd, np.float64)
        edges = []
        for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
            ab = b - a
            l2 = (ab * ab).sum(axis=-1)
            t = np.clip(np.where(l2 > 0, ((p - a) * ab).sum(axis=-1) / np.where(l2 > 0, l2, 1.0), 0.0), 0.0, 1.0)
            r = p - (a + t[..., None] * ab)
            edges.append(np.sqrt((r * r).sum(axis=-1)))
        d = np.where(np.isnan(d), np.minimum(np.minimum(edges[0], edges[1]), edges[2]), d)
        return np.where(np.isnan(d), np.inf, d).min(axis=1)


def winding_error(sd, P, w):
    """(|w - float64 winding number| (n,), which queries count, which of them lie off the surface): the queries inside the winding
    envelope (beta = +inf) whose float64 winding number is a number (a non-finite vertex makes every one a NaN); off the surface: at
    least 1e-3 of the scene's extent from every triangle, in float64.  On the surface the solid angle jumps, float32 and float64 may
    stand on different sides of a triangle and differ by a whole turn."""
    with np.errstate(**_ERR):
        w64 = scale_ref.winding64(sd, P)
        ok = _envelope(scale_ref.in_winding_envelope, sd, P, beta=INF) & np.isfinite(w64)
        err = np.abs(np.asarray(w, np.float64) - w64)
        err = np.where(ok, np.where(np.isnan(err), np.inf, err), 0.0)
        off = ok & (surface_dist64(sd, P) >= 1e-3 * scale_ref.extent(sd))
    return err, ok, off


def winding_restated(sd, P):
    """tests/winding_ref.py's float32 brute form on the device's record order (built host-only: no device is touched)."""
    import winding_ref as wr

    sc = pkg.Scene(sd, device=-1)
    try:
        tree = sc.debug_winding_tree()
    finally:
        sc.close()
    return wr.brute(wr.records(sd, tree), P, dtype=np.float32)


# ---- leg F: point sets ----
_UNIT_TRIANGLE = []


def _any_scene():
    """Point-set entries read no geometry: the scene names the device."""
    pn = np.array([[0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1]], F32)
    return pkg.scenes.SceneData(pos_nrm=pn, tri=np.array([[0, 1, 2]], np.uint32), tri_mesh=np.zeros(1, np.uint32), materials=np.ones((1, 8), F32))


def leg_points(R, c, sc, g):
    dt, fdt = pkg.POINT_NEIGHBOR_DTYPE, pkg.POINT_FRAME_DTYPE
    torch = _torch()
    data, P, n = c.data, c.points, c.n
    dD, dP, dRad = _dev(data), _dev(P), _dev(c.radius2)
    R.add("queries", n)
    R.add("cloud_" + c.kind)
    R.add(f"cloud_points_{c.m}")
    R.add("grids_cell_below_radius_8th", c.step < -3)
    R.add("grids_cell_above_8_radii", c.step > 3)
    grid = sc.point_grid_tensor(dD, c.cell)
    for mode, kw, tkw in (("scalar", dict(max_dist2=c.r2), dict(max_dist2=c.r2)), ("per-query", dict(radius2=c.radius2), dict(radius2=dRad))):
        for skip in (False, True):
            def tensor_first(k, with_counts):
                got = grid.nearest(dP, k, skip_same_index=skip, want_counts=with_counts, **tkw)
                return (_records(got[0], dt), _np(got[1])) if with_counts else (_records(got, dt), None)

            def host_first(k, with_counts):
                got = sc.nearest_points(data, c.cell, P, k, skip_same_index=skip, want_counts=with_counts, **kw)
                return got if with_counts else (got, None)

            def tensor_full():
                off, rec = grid.list(dP, skip_same_index=skip, **tkw)
                return _np(off), _records(rec, dt).reshape(-1)

            rec1, counts = _slot_leg(
                R, "points", n, POINT_K, lambda k: sc.list_point_neighbors_brute(data, P, skip_same_index=skip, k=k, **kw), host_first,
                tensor_first,
                {f"count_point_neighbors ({mode}, skip={skip})": lambda: sc.count_point_neighbors(data, c.cell, P, skip_same_index=skip, **kw),
                 f"PointGrid.count ({mode}, skip={skip})": lambda: _np(grid.count(dP, skip_same_index=skip, **tkw))},
                {f"list_point_neighbors ({mode}, skip={skip})": lambda: sc.list_point_neighbors(data, c.cell, P, skip_same_index=skip, **kw),
                 f"PointGrid.list ({mode}, skip={skip})": tensor_full}, "dist2", "index", False)
            R.add("points_total", counts.sum())
    # frames: the grid forms against the brute form, frames and neighbours
    dO = None if c.orient is None else _dev(c.orient)
    for k in c.frame_k:
        wf, wn = sc.point_frames_brute(data, P, k, radius2=c.radius2, skip_same_index=c.skip, orient=c.orient, want_neighbors=True)
        R.add("frames_short", ((wf["used"] < k) & (wf["used"] > 0)).sum())
        R.add("frames_full", (wf["used"] == k).sum())
        R.add("frames_empty", (wf["used"] == 0).sum())
        R.add("frames_tie_slots", _ties(wn, "dist2", "index"))
        got = grid.frames(dP, dD, k, radius2=dRad, skip_same_index=c.skip, orient=dO)
        R.check(f"PointGrid.frames(k={k}) frames", _records(got["records"], fdt), wf, strict=True)
        R.check(f"PointGrid.frames(k={k}) neighbours", _records(got["neighbors"], dt), wn)
        hf, hn = sc.point_frames(data, c.cell, P, k, radius2=c.radius2, skip_same_index=c.skip, orient=c.orient, want_neighbors=True)
        R.check(f"Scene.point_frames(k={k}) frames", hf, wf, strict=True)
        R.check(f"Scene.point_frames(k={k}) neighbours", hn, wn)
        wf, wn = sc.point_frames_brute(data, P, k, skip_same_index=c.skip, orient=c.orient, want_neighbors=True)  # r2 = +inf
        got = grid.knn_frames(dP, dD, k, skip_same_index=c.skip, orient=dO)
        R.check(f"PointGrid.knn_frames(k={k}) frames", _records(got["records"], fdt), wf, strict=True)
        R.check(f"PointGrid.knn_frames(k={k}) neighbours", _records(got["neighbors"], dt), wn)
        if c.m <= REF_TRIS:
            q, rad = P[:REF_QUERIES], c.radius2[:REF_QUERIES]
            o = None if c.orient is None else c.orient[:REF_QUERIES]
            df, dn = sc.point_frames_brute(data, q, k, radius2=rad, skip_same_index=c.skip, orient=o, want_neighbors=True)
            with np.errstate(**_ERR):
                rf, rn = fref.frames(q, data, k, radius2=rad, skip_same_index=c.skip, orient=o)
            R.add("ref_frames", len(q))
            R.check(f"point_frames_brute(k={k}) against point_frames_ref: frames", df, rf.astype(fdt), strict=True)
            R.check(f"point_frames_brute(k={k}) against point_frames_ref: neighbours", dn, rn.astype(dt))
    if c.m <= REF_TRIS:
        q, rad = P[:REF_QUERIES], c.radius2[:REF_QUERIES]
        for k in POINT_K:
            drec, dcnt = sc.list_point_neighbors_brute(data, q, radius2=rad, skip_same_index=c.skip, k=k)
            with np.errstate(**_ERR):
                rrec, rcnt = pnr.neighbors(q, data, radius2=rad, skip_same_index=c.skip, k=k)
            R.check(f"list_point_neighbors_brute(k={k}) against point_neighbors_ref: records", drec, rrec.astype(dt))
            R.check(f"list_point_neighbors_brute(k={k}) against point_neighbors_ref: counts", dcnt, rcnt)
        R.add("ref_point_queries", len(q))
    if c.m <= poisson_ref.MAX_N:
        pz = c.poisson
        want = sc.poisson_disk_brute(data, pz["min_dist2"], seed=pz["seed"], priority=pz["priority"])
        pr = None if pz["priority"] is None else torch.from_numpy(pz["priority"].astype(np.int64)).to(torch.int32).cuda()
        got = sc.poisson_disk_tensor(dD, pz["min_dist2"], seed=pz["seed"], priority=pr)
        R.check("poisson_disk_tensor against poisson_disk_brute", _np(got), want)
        R.check("poisson_disk against poisson_disk_brute", sc.poisson_disk(data, pz["min_dist2"], seed=pz["seed"], priority=pz["priority"]), want)
        R.add("poisson_kept", want.sum())
        R.add("poisson_dropped", (~want).sum())


LEGS = dict(A=leg_closest, B=leg_crossings, C=leg_neighbors, D=leg_sdf, E=leg_winding, F=leg_points)


def run(seed0, iterations=None, budget=None, legs=ALL, verbose=True):
    """Fuzz from seed `seed0`: `iterations` iterations of every leg in `legs` (what the tests use), or iterations until `budget`
    seconds have passed.  Returns the statistics; judges nothing.  A HIP error or a CgrtError raises and ends the run."""
    assert (iterations is None) != (budget is None), "give iterations or budget"
    import torch  # noqa: F401  (before the first call into libcgrt.so: torch's HIP runtime is the one it binds to)

    legs = [x.upper() for x in legs]
    assert legs and all(x in LEGS for x in legs), legs
    R = Run(int(seed0), verbose)
    t0 = t_last = time.time()
    any_sc = pkg.Scene(_any_scene()) if "F" in legs else None
    it = 0
    while (it < iterations) if iterations is not None else (time.time() - t0 < budget):
        R.it = it
        geometry = [x for x in legs if x != "F"]
        if geometry:
            fs = make_scene(seed0, it)
            sc = pkg.Scene(fs.sd)
            try:
                R.what = fs.describe()
                for n, leg in enumerate(geometry):
                    R.leg = leg
                    if n == 0:
                        _scene_stats(R, fs, sc)
                    LEGS[leg](R, fs, sc, _rng(seed0, it, TAG_LEG + ALL.index(leg)))
            finally:
                sc.close()
        if "F" in legs:
            c = make_cloud(seed0, it)
            R.leg, R.what = "F", f"cloud {c.kind} scale 2^{c.k} points {c.m} queries {c.n} cell 2^{c.step} radii"
            leg_points(R, c, any_sc, _rng(seed0, it, TAG_LEG + ALL.index("F")))
        it += 1
        R.stats["iterations"] = it
        if verbose and time.time() - t_last > 45:
            t_last = time.time()
            print("progress:", R.stats, flush=True)
    if any_sc is not None:
        any_sc.close()
    return R.stats


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    legs = sys.argv[3:] or ALL
    stats = run(seed0, budget=budget, legs=legs)
    print("fuzz queries:", stats, "seed", seed0, "seconds", budget, "legs", "".join(legs))
    sys.exit(1 if stats["mismatches"] else 0)

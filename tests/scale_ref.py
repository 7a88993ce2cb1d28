"""Power-of-two scaling of scenes and queries, and what the point queries owe to it (include/cgrt.h "Envelope" paragraphs of the closest-point,
crossing and signed-distance entries).  numpy only.

Multiplying every position, every query point and every ray origin by 2^k changes no significand, so inside the envelope -- no
intermediate of the definition overflows or becomes subnormal -- every float32 operation of the definitions rounds the same way: prim_id,
barycentrics, counts, orders and `inside` are unchanged, points, t and sdf are multiplied by 2^k, dist2 by 2^2k, exactly.  The predicates
below state that per record; `in_envelope` is the headers' envelope paragraph in code.  Beside them what a sign test needs: `is_closed`,
the float64 generalised winding number and queries just off the surface.
The neighbour lists share dist2's envelope (`covariant_neighbors`).  The winding numbers (5.25) have one of their own,
cubic where the others are quartic (`in_winding_envelope`, `covariant_winding_tree`): inside it w is not scaled but unchanged.
The surface attributes (5.19) have a quadratic one, per item (`surface_items`, `surface_measures`, `in_surface_envelope`,
`covariant_weights`): inside it the weights are unchanged; `covariant_samples` is the same statement for surface-sample records (5.27).
The point-set neighbours (5.30) and the Poisson-disk sets (5.29) have d2's quadratic envelope per query (`point_measures`,
`in_point_envelope`, `covariant_point_neighbors`); the iso-surfaces (5.31) a linear one per vertex-carrying edge, in the values and in the
positions separately (`in_iso_envelope`)."""
import dataclasses

import numpy as np

import closest_ref as cr

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)  # 2^-126, the smallest normal
ATAN_HEADROOM = 2.0 ** 18  # the winding numbers' upper edge: how far atan2f's smaller argument stays below FLT_MAX (see in_winding_envelope)
HEADROOM = 2.0 ** 12  # the lower edge: what stays normal below the smallest triangle's (2 * area)^2 (see in_envelope)


# ---- scaling ----
def scaled(sd, k):
    """The scene with every position multiplied by 2^k (np.ldexp: exact unless it overflows or becomes subnormal).  Normals, indices and
    everything else are untouched."""
    pn = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6).copy()
    with np.errstate(all="ignore"):
        pn[:, 0:3] = np.ldexp(pn[:, 0:3], int(k))
    return dataclasses.replace(sd, pos_nrm=pn, name=f"{sd.name}*2^{int(k)}")


def scaled_points(q, k):
    with np.errstate(all="ignore"):
        return np.ldexp(np.ascontiguousarray(np.asarray(q, np.float32).reshape(-1, 3)), int(k)).astype(np.float32)


def scaled_rays(rays, k):
    """(n, 7) rays with the origin and t multiplied by 2^k; the directions are kept."""
    r = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 7)).copy()
    with np.errstate(all="ignore"):
        r[:, 0:3] = np.ldexp(r[:, 0:3], int(k))
        r[:, 6] = np.ldexp(r[:, 6], int(k))
    return r


def _ld(x, k):
    with np.errstate(all="ignore"):
        return np.ldexp(np.asarray(x, np.float32), int(k)).astype(np.float32)


def _bits_eq(a, b):
    """Bit equality of float32 arrays, a NaN equal to a NaN (conftest.same_bits)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the covariance predicates: (n,) bool, one verdict per record ----
def covariant_closest(r0, rk, k):
    """CLOSEST_DTYPE records at scale 1 and at scale 2^k: the same prim_id and bary bits, point = ldexp(point0, k), dist2 = ldexp(dist2_0, 2k)."""
    ok = (r0["prim_id"] == rk["prim_id"]) & _bits_eq(r0["bary"], rk["bary"]).all(axis=1)
    ok &= _bits_eq(_ld(r0["point"], k), rk["point"]).all(axis=1)
    return ok & _bits_eq(_ld(r0["dist2"], 2 * k), rk["dist2"])


def covariant_crossings(ref0, refk, k):
    """(counts, offsets, records) of a full list at scale 1 and at scale 2^k (origins and t scaled, directions kept): the same count, the
    same prim_id order, t = ldexp(t0, k)."""
    (c0, o0, rec0), (ck, ok_, reck) = ref0, refk
    good = np.asarray(c0) == np.asarray(ck)
    for i in np.flatnonzero(good):
        a, b = rec0[o0[i] : o0[i + 1]], reck[ok_[i] : ok_[i + 1]]
        good[i] = bool((a["prim_id"] == b["prim_id"]).all() and _bits_eq(_ld(a["t"], k), b["t"]).all())
    return good


def covariant_first(f0, fk, k):
    """(n, m) CROSSING_DTYPE slots (first_crossings): the same ids, t = ldexp(t0, k) (+inf of an unused entry stays +inf)."""
    return ((f0["prim_id"] == fk["prim_id"]) & _bits_eq(_ld(f0["t"], k), fk["t"])).reshape(len(f0), -1).all(axis=1)


def covariant_sdf(a, b, k):
    """(sdf, inside) at scale 1 and at scale 2^k: inside equal, sdf = ldexp(sdf0, k) (sign and +-inf included)."""
    (s0, i0), (sk, ik) = a, b
    return (np.asarray(i0) == np.asarray(ik)) & _bits_eq(_ld(s0, k), sk)


def covariant_neighbors(full0, fullk, k, field="prim_id"):
    """(offsets, records) of neighbour lists (neighbors_ref.neighbors, Scene.list_neighbors; slots of any size described by their
    offsets) at scale 1 and at scale 2^k, the radius multiplied by 2^2k: the same count, the same prim_id order, dist2 = ldexp(dist2_0,
    2k) (+inf of an unused entry stays +inf).  (n,) bool, one verdict per query.  `field` names the records' id."""
    (o0, rec0), (ok_, reck) = full0, fullk
    o0, ok_ = np.asarray(o0, np.int64), np.asarray(ok_, np.int64)
    good = np.diff(o0) == np.diff(ok_)
    for i in np.flatnonzero(good):
        a, b = rec0[o0[i] : o0[i + 1]], reck[ok_[i] : ok_[i + 1]]
        good[i] = bool((a[field] == b[field]).all() and _bits_eq(_ld(a["dist2"], 2 * k), b["dist2"]).all())
    return good


def covariant_point_neighbors(full0, fullk, k):
    """covariant_neighbors for point_neighbors_ref.RECORD lists ((offsets, records) of point_neighbors_ref.neighbors, PointGrid.list):
    the same count, the same `index` order, dist2 = ldexp(dist2_0, 2k)."""
    return covariant_neighbors(full0, fullk, k, field="index")


def covariant_winding_tree(tree0, treek, k):
    """Scene.debug_winding_tree at scale 1 and at scale 2^k: the same record order and level table, every centre multiplied by 2^k,
    every r2 and every area vector by 2^2k, by bits.  One bool."""
    if not (np.array_equal(tree0["record_prims"], treek["record_prims"]) and np.array_equal(tree0["level_offsets"], treek["level_offsets"])):
        return False
    c0, ck = np.asarray(tree0["clusters"], np.float32).reshape(-1, 8), np.asarray(treek["clusters"], np.float32).reshape(-1, 8)
    if c0.shape != ck.shape:
        return False
    return bool(_bits_eq(_ld(c0[:, 0:3], k), ck[:, 0:3]).all() and _bits_eq(_ld(c0[:, 3:7], 2 * k), ck[:, 3:7]).all()
                and _bits_eq(c0[:, 7], ck[:, 7]).all())


# ---- the envelope ----
def _triangle_measures(sd):
    """(largest edge length, smallest non-zero (2 * area)^2 = |ab x ac|^2, largest |coordinate|) in float64, over finite triangles."""
    a, b, c = cr.tri_verts(sd, np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
        a, b, c = a[fin], b[fin], c[fin]
        edge = max(np.linalg.norm(b - a, axis=1).max(), np.linalg.norm(c - a, axis=1).max(), np.linalg.norm(c - b, axis=1).max())
        n = np.cross(b - a, c - a)
        area2 = (n * n).sum(axis=1)
    return float(edge), float(area2[area2 > 0].min()), float(max(np.abs(a).max(), np.abs(b).max(), np.abs(c).max()))


def in_envelope(sd, points):
    """(n,) bool: the point (a query point, or a ray's origin) lies in the envelope of the point queries on this scene -- the "Envelope"
    paragraphs of include/cgrt.h in code.  With E the scene's largest triangle edge, A the smallest non-zero (2 * area)^2 = |ab x ac|^2 of
    its triangles, S its largest |coordinate| and M(p) the largest |p - vertex| (bounded by the farthest corner of the scene's box):

      upper edge   8 * (E * M(p))^2 <= FLT_MAX       each of d1..d6 is at most E * M(p); va, vb, vc are differences of two products of
                                                     them and (va + vb) + vc sums three: none overflows.  (|cross|^2 <= E^4 and dist2 <=
                                                     3 M^2 are smaller.)
                   3 * M(p)^2 <= FLT_MAX             dist2 where E is tiny
      lower edge   A >= 2^12 * FLT_MIN               (va + vb) + vc = |ab x ac|^2 in the reals, and |cross|^2 of the crossing test is the
                                                     same quantity: it and every va, vb, vc down to 2^-12 of it stay normal
                   (2^-24 * max(S, |p|inf))^2 >= FLT_MIN   a residual of one rounding of the coordinates still has a normal square
                                                     (max(S, |p|inf) >= 2^-39)

    The upper edge is a proof for the closest-point definition.  For crossings it is not: pointInTriangle multiplies an edge by
    |p - vertex| with p the ray's hit of the triangle's PLANE, which for a grazing ray lies arbitrarily far away, so M(origin) does not
    bound it (such a product overflows only far outside the triangle, where the tests then fail through NaN as they fail in the reals).
    The lower one is a margin: cancellation can leave a non-zero va, vb or vc below 2^-12 of the sum (a weight towards an edge that small
    but not 0), which is then rounded as a subnormal; a bound that excludes it needs the granularity of the coordinates (ulp^4) and would
    put scale 1 itself outside.  tests/test_point_scale_cpu.py holds both edges to the restatements: it
    fails if covariance breaks anywhere inside.  Non-finite points are outside."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    E, A, S = _triangle_measures(sd)
    lo, hi = cr.scene_box(sd)
    with np.errstate(all="ignore"):
        far = np.maximum(np.abs(p - lo), np.abs(p - hi))
        M = np.sqrt((far * far).sum(axis=1))
        pmax = np.maximum(S, np.abs(p).max(axis=1))
        ok = np.isfinite(p).all(axis=1)
        ok &= 8.0 * (E * M) ** 2 <= FLT_MAX
        ok &= 3.0 * M * M <= FLT_MAX
        ok &= A >= HEADROOM * FLT_MIN
        ok &= (2.0 ** -24 * pmax) ** 2 >= FLT_MIN
    return ok


def _winding_measures(sd):
    """(smallest non-zero triangle edge, sum of the triangle areas, diagonal of the scene's box) in float64, over finite triangles."""
    a, b, c = cr.tri_verts(sd, np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
        a, b, c = a[fin], b[fin], c[fin]
        edges = np.concatenate([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - a, axis=1), np.linalg.norm(c - b, axis=1)])
        area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
    lo, hi = cr.scene_box(sd)
    return float(edges[edges > 0].min()), float(area), float(np.linalg.norm(hi - lo))


def nearest_vertex(sd, points, chunk_elems=1 << 22):
    """(n,) float64: the distance from every point to the nearest vertex a triangle uses (inf for a non-finite point)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    pos = np.asarray(sd.pos_nrm, np.float64).reshape(-1, 6)[:, 0:3]
    v = pos[np.unique(np.asarray(sd.tri, np.int64))]
    v = v[np.isfinite(v).all(axis=1)]
    out = np.full(len(p), np.inf)
    step = max(1, chunk_elems // max(len(v), 1))
    with np.errstate(all="ignore"):
        for s in range(0, len(p), step):
            d = p[s : s + step, None, :] - v[None]
            out[s : s + step] = np.sqrt((d * d).sum(axis=-1).min(axis=1))
    return np.where(np.isfinite(p).all(axis=1), out, np.inf)


def in_winding_envelope(sd, points, beta=2.0):
    """(n,) bool: the point lies in the envelope of the winding-number queries on this scene -- the "Envelope" paragraph of include/cgrt.h
    "Winding numbers" in code.  With M(p) the largest |p - vertex| (bounded by the farthest corner of the scene's box), m(p) the smallest
    |p - vertex|, e the smallest non-zero triangle edge, a the sum of the triangle areas and D the diagonal of the scene's box:

      upper edge   8 * M(p)^3 <= FLT_MAX             |ra|, |rb|, |rc| <= M: every product and partial sum of num = ra . (rb x rc) is at most
                                                     M^3 (Cauchy-Schwarz, |rb x rc| <= M^2), each of den's four terms is at most M^3 and
                                                     their partial sums at most 4 M^3; the factor 2 left pays for the roundings.  A centre
                                                     lies in the box, so the dipole's d2 * sqrtf(d2) <= M^3 too.
                   2 * a * M(p) <= FLT_MAX           |n| <= a for every cluster: (n.x * d.x + n.y * d.y) + n.z * d.z stays finite
                   2 * beta^2 * D^2 <= FLT_MAX       r2 <= D^2 (centre and vertices lie in the box): beta2 * r2 of the far test stays finite,
                                                     so that no cluster is opened only because its product became +inf (beta = +inf: no
                                                     condition, no cluster is ever far)
                   E^2 * M(p) <= 2^-18 * FLT_MAX     E the largest triangle edge: |num| = 2 * area * height <= E^2 * M.  atan2f is the one
                                                     operation the definition does not pin, and an implementation is scale-free only
                                                     while it need not screen its arguments: numpy's float32 arctan2 returns other bits
                                                     for (2^j y, 2^j x) than for (y, x) once |y| >= 2^123, or |x| >= 2^123 with |y| >=
                                                     2^110 (measured; den reaches 4 M^3, so only num can be kept below)
      lower edge  m(p)^3 >= FLT_MIN                 la, lb, lc >= m: (la * lb) * lc, the one term of den that nothing cancels, stays normal
                   e^3 >= 2^12 * FLT_MIN             num is six times the volume of the tetrahedron {p, v0, v1, v2} and each of its
                                                     products an edge times two distances; the three other terms of den are a dot product
                                                     times a length: a tetrahedron as small as the smallest edge in all three extents, and
                                                     every such product down to 2^-12 of its e^3, stays normal.  A far cluster has d2 > r2
                                                     >= (e / 2)^2 (a centre is not nearer than e / 2 to both ends of an edge it covers),
                                                     so d2 * sqrtf(d2) > e^3 / 8 stays normal as well.

    The upper edge is a proof but for its last line: inside it no intermediate of the definition overflows; the last line is a margin
    (ATAN_HEADROOM) for the restatement's atan2f, and says nothing about another implementation's.  Of the lower edge the first line is a proof for that
    one term; the second is a margin (HEADROOM, as for the closest points): a point in a triangle's plane has num = 0 in the reals, a right
    angle at p makes a dot product vanish, and then a non-zero product far below e^3 is rounded as a subnormal.  Excluding that needs the
    granularity of the coordinates and would put scale 1 itself outside.  Inside the envelope multiplying every position and every point
    by 2^k leaves every significand of the definition unchanged: the cluster tree is the power-of-two image (covariant_winding_tree), the
    far decisions and hence the three work counters are the same and w is the same float, bit for bit.  tests/test_query_scale_cpu.py
    holds both edges to the restatement (tests/winding_ref.py): it fails if that breaks anywhere inside.  The RECORD ORDER is not part of
    the definition -- it is the BVH builder's, whose own limits are narrower on meshes of many small triangles -- so a scale at which it
    differs from scale 1 counts as outside whatever this predicate says (that test asserts where it may not differ).  Non-finite points
    are outside."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    e, a, D = _winding_measures(sd)
    E = _triangle_measures(sd)[0]
    lo, hi = cr.scene_box(sd)
    near = nearest_vertex(sd, p)
    with np.errstate(all="ignore"):
        far = np.maximum(np.abs(p - lo), np.abs(p - hi))
        M = np.sqrt((far * far).sum(axis=1))
        ok = np.isfinite(p).all(axis=1)
        ok &= 8.0 * M ** 3 <= FLT_MAX
        ok &= 2.0 * a * M <= FLT_MAX
        if np.isfinite(beta):
            ok &= 2.0 * float(beta) ** 2 * D * D <= FLT_MAX
        ok &= E * E * M <= FLT_MAX / ATAN_HEADROOM
        ok &= near ** 3 >= FLT_MIN
        ok &= e ** 3 >= HEADROOM * FLT_MIN
    return ok


# ---- closed meshes and the winding number ----
def is_closed(sd):
    """Every directed edge of every triangle is matched exactly once by its reverse, after welding vertices with equal positions."""
    pos = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3]
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    _, weld = np.unique(pos + F32(0.0), axis=0, return_inverse=True)  # (-0 + 0 = +0: the two zeros are one position)
    t = weld.reshape(-1)[tri]
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    if (e[:, 0] == e[:, 1]).any():
        return False
    V = int(t.max()) + 1
    fwd, cnt_f = np.unique(e[:, 0] * V + e[:, 1], return_counts=True)
    rev, cnt_r = np.unique(e[:, 1] * V + e[:, 0], return_counts=True)
    return bool(len(fwd) == len(rev) and (fwd == rev).all() and (cnt_f == 1).all() and (cnt_r == 1).all())


def winding64(sd, points, chunk_elems=1 << 20):
    """(n,) float64 generalised winding number of the scene's triangles about every point: the sum of the signed solid angles (van
    Oosterom and Strackee's arctan2 form) over 4 pi.  +-1 inside a closed mesh (the sign is its orientation), 0 outside."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    a, b, c = cr.tri_verts(sd, np.float64)
    out = np.zeros(len(p))
    step = max(1, chunk_elems // max(len(a), 1))
    for s in range(0, len(p), step):
        pp = p[s : s + step, None, :]
        ra, rb, rc = a - pp, b - pp, c - pp
        la, lb, lc = (np.sqrt((x * x).sum(axis=-1)) for x in (ra, rb, rc))
        num = (ra * np.cross(rb, rc)).sum(axis=-1)
        den = la * lb * lc + (ra * rb).sum(axis=-1) * lc + (rb * rc).sum(axis=-1) * la + (rc * ra).sum(axis=-1) * lb
        out[s : s + step] = np.arctan2(num, den).sum(axis=1) / (2.0 * np.pi)
    return out


def offset_queries(sd, n, seed, h):
    """Random surface points (closest_ref.surface_queries' sampling) moved by +h (even rows) or -h (odd rows) along the float64 geometric
    normal of their triangle: just off the surface, on both sides."""
    a, b, c = cr.tri_verts(sd, np.float64)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(a), n)
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    u, v, w = 1 - r1, r1 * (1 - r2), r1 * r2
    nrm = np.cross(b[k] - a[k], c[k] - a[k])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    return (a[k] * u[:, None] + b[k] * v[:, None] + c[k] * w[:, None] + side * float(h) * nrm).astype(np.float32)


def extent(sd):
    lo, hi = cr.scene_box(sd)
    return float((hi - lo).max())


def sign_queries(sd, n, seed):
    """The point mix of the sign tests: a third uniform in the grown box, a third offset by 1e-2 of the extent, a third by 1e-3."""
    m = n // 3
    ext = extent(sd)
    return np.ascontiguousarray(np.concatenate([cr.uniform_queries(sd, m, seed), offset_queries(sd, n - 2 * m - (n - 3 * m) // 2, seed + 1, 1e-2 * ext),
                                                offset_queries(sd, m + (n - 3 * m) // 2, seed + 2, 1e-3 * ext)]), np.float32)


# ---- the surface attributes (include/cgrt.h cgrt_hit_barycentrics*, "Envelope") ----
def surface_items(sd, n, seed):
    """(rays (n, 7) float32, prim (n,) int64): n hits made without a tracer.  The points and their triangles are sampling_ref.sample(sd, n,
    seed)'s; item i with i % 8 == 1 has the weight of v0 moved onto v1 (a point on the edge v1 v2), item i with i % 16 == 2 the weights
    (0, 0, 1) (the vertex v2), their points recomputed by the same float32 mix.  Unit directions and t in [0.5, 2] extents are drawn
    from np.random.default_rng(seed); the origin is float32(p - d * t), so that o + d * t lands on p up to rounding.  t is rays[:, 6]."""
    import sampling_ref

    rec, _ = sampling_ref.sample(sd, n, seed)
    prim = rec["prim_id"].astype(np.int64)
    bary = rec["bary"].copy()
    i = np.arange(n)
    edge, vertex = i % 8 == 1, i % 16 == 2
    bary[edge] = np.stack([np.zeros(int(edge.sum()), F32), bary[edge, 0] + bary[edge, 1], bary[edge, 2]], axis=1)
    bary[vertex] = (0.0, 0.0, 1.0)
    v0, v1, v2 = (v[prim] for v in sampling_ref.vertices(sd))
    p = (bary[:, 0:1] * v0 + bary[:, 1:2] * v1) + bary[:, 2:3] * v2
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    t = (rng.uniform(0.5, 2.0, n) * extent(sd)).astype(F32)
    rays = np.empty((n, 7), F32)
    rays[:, 0:3] = (p.astype(np.float64) - d.astype(np.float64) * t.astype(np.float64)[:, None]).astype(F32)
    rays[:, 3:6], rays[:, 6] = d, t
    return rays, prim


def _span(parts):
    """(smallest non-zero magnitude, largest magnitude) per row, in float64, over float32 arrays of n rows (+inf and 0 for a row of zeros)."""
    a = np.abs(np.concatenate([np.asarray(x, np.float64).reshape(len(x), -1) for x in parts], axis=1))
    return np.where(a > 0, a, np.inf).min(axis=1), a.max(axis=1)


def surface_measures(sd, rays, prim):
    """(min_lin, max_lin, min_quad, max_quad), each (n,) float64: the smallest non-zero and the largest magnitude of the float32
    intermediates of the weights' definition (tests/surface_ref.py) at scale 1, per item.
      linear     (multiplied by 2^k under a scale of 2^k)   o, d * t, p = o + d * t, the three vertices, and the two edge differences each
                 of the four areas takes: of (v0, v1, v2), (p, v1, v2), (p, v0, v2) and (p, v0, v1)
      quadratic  (multiplied by 2^2k)   the six products and the three components of each cross product, each magnitude as narrowed to
                 float32, and each area
    A zero stays a zero at every scale and is left out of the minimum.  The magnitude's squares and their sum are taken in double, where
    nothing a float32 can hold overflows or is lost, so nothing of the fourth degree enters."""
    import surface_ref

    r = np.ascontiguousarray(np.asarray(rays, F32).reshape(-1, 7))
    o, d, t = r[:, 0:3], r[:, 3:6], r[:, 6]
    _, (v0, v1, v2), _ = surface_ref.triangle_vertices(sd, np.asarray(prim, np.int64))
    with np.errstate(all="ignore"):
        dt = d * t[:, None]
        p = o + dt
        lin, quad = [o, dt, p, v0, v1, v2], []
        for a, b, c in ((v0, v1, v2), (p, v1, v2), (p, v0, v2), (p, v0, v1)):
            e1, e2 = b - a, c - a
            lin += [e1, e2]
            x = surface_ref._cross(e1, e2)
            mag = surface_ref.magnitude(x)
            quad += [e1[:, 1] * e2[:, 2], e2[:, 1] * e1[:, 2], e1[:, 2] * e2[:, 0], e2[:, 2] * e1[:, 0], e1[:, 0] * e2[:, 1], e2[:, 0] * e1[:, 1],
                     x, mag, mag / F32(2.0)]
    return _span(lin) + _span(quad)


def in_surface_envelope(measures, k):
    """(n,) bool: the item lies in the envelope of the surface attributes at scale 2^k -- the "Envelope" paragraph of include/cgrt.h's
    surface-attribute entries in code: every linear intermediate of its definition times 2^k, and every quadratic one times 2^2k, is a
    normal float32 (or zero).  Quadratic where the point queries are quartic and the winding numbers cubic.  Inside, every float32
    operation of the definition rounds as at scale 1 and the two operands of each ratio carry the same factor 2^2k: the weights have the
    bits they have at scale 1."""
    min_lin, max_lin, min_quad, max_quad = measures
    k = int(k)
    with np.errstate(all="ignore"):
        return ((np.ldexp(min_lin, k) >= FLT_MIN) & (np.ldexp(max_lin, k) <= FLT_MAX)
                & (np.ldexp(min_quad, 2 * k) >= FLT_MIN) & (np.ldexp(max_quad, 2 * k) <= FLT_MAX))


def covariant_weights(w0, wk):
    """(n, 3) weights at scale 1 and at scale 2^k: the same bits (a NaN equal to a NaN), whatever k is."""
    return _bits_eq(w0, wk).reshape(len(w0), -1).all(axis=1)


def covariant_samples(r0, rk, k):
    """Surface-sample records (sampling_ref.SAMPLE_DTYPE) at scale 1 and at scale 2^k: the same prim_id, mesh_id and bary bits, point =
    ldexp(point0, k)."""
    ok = (r0["prim_id"] == rk["prim_id"]) & (r0["mesh_id"] == rk["mesh_id"]) & _bits_eq(r0["bary"], rk["bary"]).all(axis=1)
    return ok & _bits_eq(_ld(r0["point"], k), rk["point"]).all(axis=1)


# ---- point sets (include/cgrt.h "Point-set neighbours" and "Poisson-disk sets", "Envelope") ----
def point_measures(points, data, block=256):
    """(min_dx, max_d2, finite), each (n,): per query, in float64 from the float32 inputs, the smallest non-zero |q.c - d_j.c| over all
    finite data points j and the three axes (+inf where there is none), the largest exact squared distance to a finite data point (0
    where there is none), and whether the query is finite."""
    q = np.asarray(points, F32).reshape(-1, 3).astype(np.float64)
    d = np.asarray(data, F32).reshape(-1, 3).astype(np.float64)
    d = d[np.isfinite(d).all(axis=1)]
    fin = np.isfinite(q).all(axis=1)
    min_dx, max_d2 = np.full(len(q), np.inf), np.zeros(len(q))
    if len(d) == 0:
        return min_dx, max_d2, fin
    with np.errstate(all="ignore"):
        for s in range(0, len(q), block):
            dx = np.abs(np.where(fin[s : s + block, None, None], q[s : s + block, None, :], 0.0) - d[None])
            max_d2[s : s + block] = (dx * dx).sum(axis=-1).max(axis=1)
            min_dx[s : s + block] = np.where(dx > 0, dx, np.inf).min(axis=(1, 2))
    return min_dx, np.where(fin, max_d2, 0.0), fin


def in_point_envelope(measures, r2, k):
    """(n,) bool: the query lies in the envelope of the point-set queries at scale 2^k (data, queries by 2^k; r2, the scale-1 bound, a
    scalar or (n,), by 2^2k) -- the "Envelope" paragraph of include/cgrt.h "Point-set neighbours" in code:

      lower edge   min|dx|^2 * 2^2k >= FLT_MIN   the smallest non-zero coordinate difference still has a normal square: every dx, every
                                                 product and both sums are normal or zero
      upper edge   max d2 * 2^2k <= FLT_MAX      no d2 to any data point overflows, hence no product or partial sum
      bound        r2 * 2^2k is a normal float   (finite, not zero, not subnormal: the comparison `d2 <= r2` sees the image of r2)
      the query and r2 are finite

    Inside it every float32 operation of d2 rounds as at scale 1: d2 is multiplied by 2^2k exactly, membership and order are unchanged."""
    min_dx, max_d2, fin = measures
    k = int(k)
    r = np.broadcast_to(np.asarray(r2, np.float64), fin.shape)
    with np.errstate(all="ignore"):
        rk = np.ldexp(r, 2 * k)
        ok = fin & np.isfinite(r) & (rk >= FLT_MIN) & (rk <= FLT_MAX)
        ok &= np.ldexp(min_dx * min_dx, 2 * k) >= FLT_MIN
        ok &= np.ldexp(max_d2, 2 * k) <= FLT_MAX
    return ok


# ---- iso-surfaces (include/cgrt.h "Iso-surfaces", "Envelope") ----
def _normal_or_zero(x, k):
    """x (float32 magnitudes at scale 1) times 2^k, taken in float64: zero, or a normal float32."""
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(all="ignore"):
        s = np.ldexp(a, int(k))
        return (a == 0) | ((s >= FLT_MIN) & (s <= FLT_MAX))


def in_iso_envelope(values, iso, origin, spacing, dims, kv, kp, inside_above=False):
    """(nv,) bool, one verdict per vertex-carrying edge in the vertex order: the edge lies in the envelope of the iso-surface at values and
    iso times 2^kv and origin and spacing times 2^kp -- the "Envelope" paragraph of include/cgrt.h "Iso-surfaces" in code.  Every non-zero
    one of these float32 intermediates of the definition, taken at scale 1, stays a normal float:
      times 2^kv   vA, vB, iso, fl(iso - vA), fl(vB - vA)
      times 2^kp   per component: both ends' grid positions with their products (float)i * spacing.c, fl(pB.c - pA.c), fl(t fl(pB.c - pA.c))
                   and the vertex's coordinate
    Inside it t has the bits it has at scale 1 (both operands of the ratio carry 2^kv) and every coordinate is multiplied by 2^kp exactly.
    Non-finite origin, spacing or iso: outside."""
    import isosurface_ref as iref

    v = np.ascontiguousarray(np.asarray(values, F32))
    nz, ny, nx = v.shape
    assert (nx, ny, nz) == tuple(int(x) for x in dims)
    o, sp = np.asarray(origin, F32).reshape(3), np.asarray(spacing, F32).reshape(3)
    iso = F32(iso)
    owner, etype = iref.carrying_edges(v, iso, inside_above)
    d = iref.CORNERS[etype + 1]
    idx = [owner % nx, (owner // nx) % ny, owner // (nx * ny)]
    flat = v.reshape(-1)
    vA, vB = flat[owner], flat[owner + d[:, 0] + d[:, 1] * nx + d[:, 2] * nx * ny]
    ok = np.full(len(owner), bool(np.isfinite(iso) and np.isfinite(o).all() and np.isfinite(sp).all()))
    with np.errstate(all="ignore"):
        t = (iso - vA) / (vB - vA)
        t = np.where(t >= F32(0), t, F32(0)).astype(F32)
        t = np.where(t > F32(1), F32(1), t).astype(F32)
        for x in (vA, vB, np.full(len(owner), iso, F32), iso - vA, vB - vA):
            ok &= _normal_or_zero(x, kv)
        for c in range(3):
            iA, iB = idx[c].astype(F32), (idx[c] + d[:, c]).astype(F32)
            pA, pB = o[c] + iA * sp[c], o[c] + iB * sp[c]
            diff = pB - pA
            for x in (np.full(len(owner), o[c], F32), iA * sp[c], iB * sp[c], pA, pB, diff, t * diff, pA + t * diff):
                ok &= _normal_or_zero(x, kp)
    return ok

"""numpy restatement of the closest-point definition (include/cgrt.h "Closest-point queries"), written from that text:
float32, every operation rounded, vectorised over triangles, the regions selected with np.where in the stated priority.  Beside it the
brute-force selection (smallest dist2 <= max_dist2, ties to the smaller prim_id), the box lower bound of the lemma, a float64 referee (the
same region walk in float64, without the clamp) and the seeded query families of the tests."""
import numpy as np

F32 = np.float32
NO_PRIM = 0xFFFFFFFF
CLOSEST_DTYPE = np.dtype([("point", np.float32, 3), ("dist2", np.float32), ("prim_id", np.uint32), ("bary", np.float32, 3)])


def tri_verts(sd, dtype=np.float32):
    """a, b, c: (T, 3) positions of tri[:, 0..2] (the f32 values given to cgrt_scene_create)."""
    pos = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3]
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    return tuple(np.ascontiguousarray(pos[tri[:, k]].astype(dtype)) for k in range(3))


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _walk(p, a, b, c, one, zero):
    """The region walk in the dtype of the operands: v, w and the unclamped q.  Shapes broadcast; the last axis is xyz."""
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    rA = (d1 <= 0) & (d2 <= 0)
    rB = (d3 >= 0) & (d4 <= d3)
    rAB = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    rC = (d6 >= 0) & (d5 <= d6)
    rAC = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    rBC = (va <= 0) & (e1 >= 0) & (e2 >= 0)
    den = one / ((va + vb) + vc)
    w_bc = e1 / (e1 + e2)
    v = vb * den
    w = vc * den
    v = np.where(rBC, one - w_bc, v)
    w = np.where(rBC, w_bc, w)
    v = np.where(rAC, zero, v)
    w = np.where(rAC, d2 / (d2 - d6), w)
    v = np.where(rC, zero, v)
    w = np.where(rC, one, w)
    v = np.where(rAB, d1 / (d1 - d3), v)
    w = np.where(rAB, zero, w)
    v = np.where(rB, one, v)
    w = np.where(rB, zero, w)
    v = np.where(rA, zero, v)
    w = np.where(rA, zero, w)
    q = (a + ab * v[..., None]) + ac * w[..., None]
    atA, atB, atC = rA, ~rA & rB, ~rA & ~rB & ~rAB & rC
    q = np.where(atC[..., None], c, q)
    q = np.where(atB[..., None], b, q)
    q = np.where(atA[..., None], a, q)
    return v, w, q


def closest_tri32(p, a, b, c):
    """The definition for points p against triangles (a, b, c), broadcast (e.g. p (Q, 1, 3) against (T, 3)).  float32.
    Returns q, dist2, u, v, w."""
    p, a, b, c = (np.asarray(x, np.float32) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        v, w, q = _walk(p, a, b, c, F32(1.0), F32(0.0))
        u = (F32(1.0) - v) - w
        lo = np.minimum(np.minimum(a, b), c)
        hi = np.maximum(np.maximum(a, b), c)
        q = np.where(q < lo, lo, np.where(q > hi, hi, q))
        r = p - q
        dist2 = _dot(r, r)
    assert q.dtype == np.float32 and dist2.dtype == np.float32 and u.dtype == np.float32
    return q, dist2, u, v, w


def miss_records(n):
    out = np.zeros(n, CLOSEST_DTYPE)
    out["dist2"] = np.inf
    out["prim_id"] = NO_PRIM
    return out


def brute(sd, points, max_dist2=np.inf, chunk_elems=1 << 18):
    """The result of every query by the definition: CLOSEST_DTYPE records."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    out = miss_records(len(p))
    T = int(np.asarray(sd.tri).reshape(-1, 3).shape[0])
    if T == 0 or len(p) == 0:
        return out
    a, b, c = tri_verts(sd)
    step = max(1, chunk_elems // T)
    md = F32(max_dist2)
    for s in range(0, len(p), step):
        pp = p[s : s + step]
        q, d2, u, v, w = closest_tri32(pp[:, None, :], a, b, c)
        ok = d2 <= md  # (a NaN never qualifies)
        best = np.where(ok, d2, F32(np.inf)).min(axis=1)
        cand = ok & (d2 == best[:, None])
        k = cand.argmax(axis=1)  # the first candidate: the smallest prim_id
        hit = cand.any(axis=1) & np.isfinite(pp).all(axis=1)
        rows = np.arange(len(pp))
        o = out[s : s + step]
        o["point"][hit] = q[rows, k][hit]
        o["dist2"][hit] = d2[rows, k][hit]
        o["prim_id"][hit] = k[hit].astype(np.uint32)
        o["bary"][hit] = np.stack([u[rows, k], v[rows, k], w[rows, k]], axis=1)[hit]
    return out


def box_lb2(lo, hi, p):
    """Squared distance from p to the box [lo, hi] in dist2's float32 operations and association (broadcast; last axis xyz)."""
    lo, hi, p = (np.asarray(x, np.float32) for x in (lo, hi, p))
    with np.errstate(all="ignore"):
        d = np.maximum(np.maximum(lo - p, p - hi), F32(0.0))
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dist64(sd, points, chunk_elems=1 << 18):
    """The float64 referee: (Q, T) distances |p - q| of the same region walk in float64, without the clamp."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    a, b, c = tri_verts(sd, np.float64)
    T = len(a)
    out = np.empty((len(p), T), np.float64)
    step = max(1, chunk_elems // max(T, 1))
    with np.errstate(all="ignore"):
        for s in range(0, len(p), step):
            pp = p[s : s + step, None, :]
            _, _, q = _walk(pp, a, b, c, 1.0, 0.0)
            r = pp - q
            out[s : s + step] = np.sqrt(_dot(r, r))
    return out


def scene_scale(sd):
    pos = np.asarray(sd.pos_nrm, np.float64).reshape(-1, 6)[:, 0:3]
    used = pos[np.unique(np.asarray(sd.tri, np.int64))]
    return float(np.abs(used[np.isfinite(used)]).max())


# ---- query families (seeded) ----
def scene_box(sd):
    a, b, c = tri_verts(sd)
    v = np.concatenate([a, b, c]).astype(np.float64)
    v = np.where(np.isfinite(v), v, np.nan)
    return np.nanmin(v, axis=0), np.nanmax(v, axis=0)


def uniform_queries(sd, n, seed):
    """Uniform in the scene box grown by 25 % (of its extent, on every side)."""
    lo, hi = scene_box(sd)
    ext = np.maximum(hi - lo, 1e-3)
    rng = np.random.default_rng(seed)
    return (lo - 0.25 * ext + rng.random((n, 3)) * (1.5 * ext)).astype(np.float32)


def surface_queries(sd, n, seed):
    """Points on random triangles (random barycentrics, rounded to float32: on the surface up to rounding)."""
    a, b, c = tri_verts(sd, np.float64)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(a), n)
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    u, v, w = 1 - r1, r1 * (1 - r2), r1 * r2
    return (a[k] * u[:, None] + b[k] * v[:, None] + c[k] * w[:, None]).astype(np.float32)


def vertex_queries(sd, n, seed):
    """Exact vertex positions of random triangles: every triangle sharing the vertex ties at dist2 == 0."""
    a, b, c = tri_verts(sd)
    rng = np.random.default_rng(seed)
    k, which = rng.integers(0, len(a), n), rng.integers(0, 3, n)
    return np.stack([a, b, c], axis=1)[k, which].copy()


def edge_queries(sd, n, seed):
    """Edge midpoints of random triangles (float32)."""
    a, b, c = tri_verts(sd)
    rng = np.random.default_rng(seed)
    k, which = rng.integers(0, len(a), n), rng.integers(0, 3, n)
    v = np.stack([a, b, c], axis=1)[k]
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        return (F32(0.5) * v[rows, which] + F32(0.5) * v[rows, (which + 1) % 3]).astype(np.float32)


def far_queries(sd, n, seed):
    """Far points: 100 x the scene's extent away from its centre, in random directions."""
    lo, hi = scene_box(sd)
    ext = max(float((hi - lo).max()), 1e-3)
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (0.5 * (lo + hi) + 100.0 * ext * d).astype(np.float32)


def mixed_queries(sd, n, seed):
    """The five families interleaved (query i belongs to family i % 5), then one NaN point at index 5 and one inf point at index 6
    (where the list is long enough): every prefix of 7 or more holds all of them."""
    m = (n + 4) // 5
    fams = [uniform_queries(sd, m, seed), surface_queries(sd, m, seed + 1), vertex_queries(sd, m, seed + 2), edge_queries(sd, m, seed + 3),
            far_queries(sd, m, seed + 4)]
    q = np.stack(fams, axis=1).reshape(-1, 3)[:n].copy()
    if n > 5:
        q[5, 1] = np.nan
    if n > 6:
        q[6, 2] = np.inf
    return np.ascontiguousarray(q, np.float32)

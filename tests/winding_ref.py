"""The definition of the winding-number queries (include/cgrt.h "Winding numbers") on the CPU, written from that text.
numpy only.

* `records`       the triangles in record order, from the record order Scene.debug_winding_tree reports.
* `clusters`      the cluster tree over them in float64: per level the centres, area vectors and sums of |area vector|.
* `walk`          the tree form.  The far decisions are evaluated in np.float32 in the header's operation order -- they ARE the definition,
                  so the three work counters are reproducible here --, the values in `dtype` (float64: what the walk is worth; float32: the
                  header's arithmetic, every operation rounded on its own, the additions in the walk's order).
* `brute`         every triangle in record order.
Both return w; `walk` also the counters (clusters tested, dipoles taken, triangles evaluated)."""
import numpy as np

F32 = np.float32
INV_4PI = 0.07957747154594767  # 1 / (4 pi); the header rounds it to f32


def level_counts(ntris):
    """Clusters per level, level 0 first: ceil(previous / 8) down to the first level with at most 8."""
    counts, c = [], int(ntris)
    while c > 0:
        c = -(-c // 8)
        counts.append(c)
        if c <= 8:
            break
    return counts


def records(sd, tree):
    """(ntris, 3, 3) float32: the vertices of every triangle record in record order."""
    pos = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3]
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    return np.ascontiguousarray(pos[tri[np.asarray(tree["record_prims"], np.int64)]], np.float32)


def clusters(recs):
    """The tree in float64 from the records: a list of levels, each {'c': (m, 3) centres, 'n': (m, 3) summed area vectors, 'abs': (m,) sums
    of |area vector|, 'first', 'last': (m,) the records [first, last) a cluster covers}."""
    v = np.asarray(recs, np.float64)
    with np.errstate(all="ignore"):
        nv = 0.5 * np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        area = np.sqrt((nv * nv).sum(axis=1))
        cen = v.sum(axis=1) / 3.0
    T = len(v)
    out = []
    for L, m in enumerate(level_counts(T)):
        span = 8 ** (L + 1)
        first = np.arange(m, dtype=np.int64) * span
        last = np.minimum(first + span, T)
        lvl = {"c": np.zeros((m, 3)), "n": np.zeros((m, 3)), "abs": np.zeros(m), "first": first, "last": last}
        for i in range(m):
            s = slice(first[i], last[i])
            with np.errstate(all="ignore"):
                a = area[s].sum()
                lvl["n"][i] = nv[s].sum(axis=0)
                lvl["abs"][i] = a
                lvl["c"][i] = (area[s, None] * cen[s]).sum(axis=0) / a if (a > 0 and np.isfinite(a)) else cen[s].mean(axis=0)
        out.append(lvl)
    return out


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def omega(v, p):
    """2 * atan2(num, den) of the triangles v (..., 3, 3) seen from the points p (..., 3), in the arrays' dtype, the header's association."""
    dt = v.dtype.type
    with np.errstate(all="ignore"):
        ra, rb, rc = v[..., 0, :] - p, v[..., 1, :] - p, v[..., 2, :] - p
        la, lb, lc = np.sqrt(_dot(ra, ra)), np.sqrt(_dot(rb, rb)), np.sqrt(_dot(rc, rc))
        u = np.stack([rb[..., 1] * rc[..., 2] - rb[..., 2] * rc[..., 1], rb[..., 2] * rc[..., 0] - rb[..., 0] * rc[..., 2],
                      rb[..., 0] * rc[..., 1] - rb[..., 1] * rc[..., 0]], axis=-1)
        num = _dot(ra, u)
        den = (((la * lb) * lc + _dot(ra, rb) * lc) + _dot(rb, rc) * la) + _dot(rc, ra) * lb
        out = dt(2.0) * np.arctan2(num, den)
    assert out.dtype == v.dtype
    return out


def _ordered_sum(n, pts, keys, vals, dtype):
    """acc[i] = the sum of point i's contributions, added one at a time in ascending key order (the walk's order) in `dtype`."""
    acc = np.zeros(n, dtype)
    if len(pts) == 0:
        return acc
    order = np.lexsort((keys, pts))
    pts, vals = pts[order], vals[order]
    rank = np.arange(len(pts)) - np.searchsorted(pts, pts, side="left")
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(rank))])
    with np.errstate(all="ignore"):
        for j in range(len(bounds) - 1):
            sel = by_rank[bounds[j] : bounds[j + 1]]  # (every point at most once)
            acc[pts[sel]] = acc[pts[sel]] + vals[sel]
    assert acc.dtype == dtype
    return acc


def walk(tree, recs, points, beta, dtype=np.float64, chunk=1 << 20):
    """The tree form on the device's tree (Scene.debug_winding_tree).  Returns (w (n,) dtype, (clusters tested, dipoles taken, triangles
    evaluated))."""
    dtype = np.dtype(dtype)
    p32 = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    pd = p32.astype(dtype)
    n, T = len(p32), len(recs)
    cl = np.asarray(tree["clusters"], np.float32).reshape(-1, 8)
    off = [int(x) for x in tree["level_offsets"]]
    counts = level_counts(T)
    assert [off[k + 1] - off[k] for k in range(len(off) - 1)] == counts, "the level table is not the one the triangle count gives"
    work = [0, 0, 0]
    if T == 0 or n == 0:
        return np.zeros(n, dtype), tuple(work)
    with np.errstate(all="ignore"):
        beta2 = F32(beta) * F32(beta)  # rounded once
    rv = np.asarray(recs, np.float32).astype(dtype)
    finite = np.isfinite(p32).all(axis=1)
    top = len(counts) - 1
    vis_p = np.repeat(np.flatnonzero(finite), counts[top])
    vis_c = np.tile(np.arange(counts[top]), int(finite.sum()))
    P, K, V = [], [], []
    for L in range(top, -1, -1):
        C = cl[off[L] : off[L + 1]]
        with np.errstate(all="ignore"):
            d = C[vis_c, 0:3] - p32[vis_p]
            d2 = _dot(d, d)
            assert d2.dtype == np.float32
            far = d2 > beta2 * C[vis_c, 3]  # (false for a NaN)
        work[0] += len(vis_p)
        work[1] += int(far.sum())
        fp, fc = vis_p[far], vis_c[far]
        with np.errstate(all="ignore"):
            dd = C[fc, 0:3].astype(dtype) - pd[fp]
            dd2 = _dot(dd, dd)
            val = _dot(C[fc, 4:7].astype(dtype), dd) / (dd2 * np.sqrt(dd2))
        P.append(fp), K.append(fc.astype(np.int64) * 8 ** (L + 1)), V.append(val.astype(dtype, copy=False))
        np_, nc = vis_p[~far], vis_c[~far]
        limit = counts[L - 1] if L > 0 else T
        child = nc[:, None].astype(np.int64) * 8 + np.arange(8)
        ok = child < limit
        vis_p, vis_c = np.repeat(np_, 8).reshape(-1, 8)[ok], child[ok]
    work[2] = len(vis_p)  # (point, record) pairs of the opened level-0 clusters
    for s in range(0, len(vis_p), chunk):
        tp, tk = vis_p[s : s + chunk], vis_c[s : s + chunk]
        P.append(tp), K.append(tk), V.append(omega(rv[tk], pd[tp]))
    acc = _ordered_sum(n, np.concatenate(P), np.concatenate(K), np.concatenate(V), dtype)
    with np.errstate(all="ignore"):
        w = acc * dtype.type(INV_4PI)  # (float32: the header's constant)
    assert w.dtype == dtype
    return w, tuple(work)


def brute(recs, points, dtype=np.float64, chunk=256):
    """The brute form: acc += omega_k for k in record order, in `dtype`; a non-finite point gets 0."""
    dtype = np.dtype(dtype)
    pd = np.asarray(points, np.float32).reshape(-1, 3).astype(dtype)
    rv = np.asarray(recs, np.float32).astype(dtype)
    finite = np.isfinite(pd).all(axis=1)
    acc = np.zeros(len(pd), dtype)
    q = pd[finite]
    a = np.zeros(len(q), dtype)
    with np.errstate(all="ignore"):
        for s in range(0, len(rv), chunk):
            om = omega(rv[None, s : s + chunk], q[:, None, :])  # (points, chunk)
            for k in range(om.shape[1]):
                a = a + om[:, k]
        acc[finite] = a
        w = acc * dtype.type(INV_4PI)  # (float32: the header's constant)
    assert w.dtype == dtype
    return w

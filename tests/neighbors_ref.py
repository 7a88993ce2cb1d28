"""numpy restatement of the neighbour queries (include/cgrt.h "Neighbour queries"), written from that text on top of
closest_ref.closest_tri32 (the restatement of dist2): membership (`dist2 <= r2` is true; a radius for which `r2 >= 0` is false and a
non-finite point have no neighbours), the (dist2, prim_id) order, and the slot rule with its clamping."""
import numpy as np

import closest_ref as cr

F32 = np.float32
NO_PRIM = 0xFFFFFFFF
NEIGHBOR_DTYPE = np.dtype([("dist2", np.float32), ("prim_id", np.uint32)])
UNUSED = np.array([(np.inf, NO_PRIM)], NEIGHBOR_DTYPE)[0]


def extent(sd):
    """The largest side of the scene's box."""
    lo, hi = cr.scene_box(sd)
    return float((hi - lo).max())


def bounds(n, radius2=None, max_dist2=np.inf):
    """r2 of every query: radius2[i], or max_dist2."""
    if radius2 is None:
        return np.full(n, max_dist2, np.float32)
    r = np.asarray(radius2, np.float32).reshape(-1)
    assert len(r) == n
    return r


def membership(sd, points, r2, chunk_elems=1 << 18, dist2=None):
    """Yields (first query, dist2 (q, T) float32, member (q, T) bool) for chunks of the queries.  dist2: a dict that keeps every chunk's
    dist2 for a later call on the same scene and points (another radius); the chunks are not changed."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
    T = int(np.asarray(sd.tri).reshape(-1, 3).shape[0])
    if T == 0 or len(p) == 0:
        return
    a, b, c = cr.tri_verts(sd)
    step = max(1, chunk_elems // T)
    with np.errstate(all="ignore"):
        for s in range(0, len(p), step):
            pp, rr = p[s : s + step], r2[s : s + step]
            if dist2 is not None and s in dist2:
                d2 = dist2[s]
            else:
                _, d2, _, _, _ = cr.closest_tri32(pp[:, None, :], a, b, c)
                if dist2 is not None:
                    dist2[s] = d2
            live = np.isfinite(pp).all(axis=1) & (rr >= F32(0.0))  # (a NaN radius compares false)
            yield s, d2, (d2 <= rr[:, None]) & live[:, None]  # (a NaN dist2 never qualifies)


def neighbors(sd, points, radius2=None, max_dist2=np.inf, dist2=None):
    """The full answer by the definition: (offsets (n + 1,) int64, records NEIGHBOR_DTYPE) -- query i's neighbours, in (dist2, prim_id)
    order, are records[offsets[i]:offsets[i + 1]]; its count is offsets[i + 1] - offsets[i].  dist2: membership's."""
    n = len(np.asarray(points, np.float32).reshape(-1, 3))
    counts = np.zeros(n, np.int64)
    parts = []
    for s, d2, ok in membership(sd, points, bounds(n, radius2, max_dist2), dist2=dist2):
        counts[s : s + len(ok)] = ok.sum(axis=1)
        rows, prims = np.nonzero(ok)
        d = d2[rows, prims]
        order = np.lexsort((prims, d, rows))  # by query, then dist2 as floats, then prim_id
        rec = np.zeros(len(order), NEIGHBOR_DTYPE)
        rec["dist2"], rec["prim_id"] = d[order], prims[order]
        parts.append(rec)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, (np.concatenate(parts) if parts else np.zeros(0, NEIGHBOR_DTYPE))


def fill_slots(full, out, offsets=None, k=0):
    """The slot rule on `out` (capacity = len(out) records, changed in place and returned): query i owns [offsets[i], offsets[i + 1]) --
    a decreasing pair is an empty slot, both ends are clamped to the capacity -- or [i * k, (i + 1) * k); a slot of s records receives
    the first min(s, count) neighbours of `full` (what neighbors() returned) in order and {+inf, NO_PRIM} in its remaining entries.
    Nothing else is written.  Slots are filled in query order (overlapping slots have no defined result: do not test them)."""
    foff, frec = full
    n, cap = len(foff) - 1, len(out)
    assert (offsets is not None) != (k > 0)
    for i in range(n):
        if offsets is not None:
            b, e = int(offsets[i]), int(offsets[i + 1])
            e = max(e, b)
        else:
            b, e = i * k, (i + 1) * k
        b, e = min(b, cap), min(e, cap)
        m = min(e - b, int(foff[i + 1] - foff[i]))
        out[b : b + m] = frec[foff[i] : foff[i] + m]
        out[b + m : e] = UNUSED
    return out


def nearest(full, k):
    """(n, k) records: the k nearest of every query."""
    n = len(full[0]) - 1
    return fill_slots(full, np.zeros(n * k, NEIGHBOR_DTYPE), k=k).reshape(n, k)


def same(a, b):
    """Two NEIGHBOR_DTYPE arrays, byte for byte."""
    return a.shape == b.shape and a.dtype == b.dtype == NEIGHBOR_DTYPE and a.tobytes() == b.tobytes()


def first_difference(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    if len(a) != len(b):
        return ("lengths", len(a), len(b))
    for i in np.flatnonzero((a["dist2"].view(np.uint32) != b["dist2"].view(np.uint32)) | (a["prim_id"] != b["prim_id"]))[:1]:
        return int(i), a[i], b[i]
    return None

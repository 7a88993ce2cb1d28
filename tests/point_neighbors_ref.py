"""Point-set neighbours (include/cgrt.h "Point-set neighbours") restated in numpy from their definition -- not from the
library's sources.  Not a test module; numpy only.  O(n m), no grid: an all-pairs matrix, computed in row blocks.

  * d2_matrix(): fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) with dx = fl(q.x - d.x), every operation rounded on its own (numpy float32
    arithmetic does not contract);
  * members(): both points finite, `d2 <= r2` true (a NaN or negative r2: nobody), index j != i under skip_same_index;
  * neighbors(): the per-query lists by a stable sort on (d2, index), and the slot rule -- k records per query, or caller offsets."""
import numpy as np

F32 = np.float32
NO_PRIM = 0xFFFFFFFF
RECORD = np.dtype([("dist2", np.float32), ("index", np.uint32)])
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def finite(points):
    return np.isfinite(np.asarray(points, F32).reshape(-1, 3)).all(1)


def d2_matrix(points, data):
    """(n, m) float32."""
    q, d = np.asarray(points, F32).reshape(-1, 3), np.asarray(data, F32).reshape(-1, 3)
    with np.errstate(**_ERR):
        dx = [q[:, None, k] - d[None, :, k] for k in range(3)]
        assert all(x.dtype == F32 for x in dx)
        return (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]


def bounds(n, radius2=None, max_dist2=np.inf):
    """(n,) float32: r2 per query."""
    if radius2 is None:
        return np.full(n, max_dist2, F32)
    r = np.asarray(radius2, F32).reshape(-1)
    assert r.shape == (n,)
    return r


def members(points, data, radius2=None, max_dist2=np.inf, skip_same_index=False, d2=None):
    """((n, m) bool, the d2 matrix)."""
    q, d = np.asarray(points, F32).reshape(-1, 3), np.asarray(data, F32).reshape(-1, 3)
    d2 = d2_matrix(q, d) if d2 is None else d2
    r2 = bounds(len(q), radius2, max_dist2)
    with np.errstate(**_ERR):
        mem = (d2 <= r2[:, None]) & (r2 >= 0)[:, None]  # (a NaN on either side compares false)
    mem &= finite(q)[:, None] & finite(d)[None, :]
    if skip_same_index:
        k = min(len(q), len(d))
        mem[np.arange(k), np.arange(k)] = False
    return mem, d2


def neighbors(points, data, radius2=None, max_dist2=np.inf, skip_same_index=False, k=0, offsets=None, block=512):
    """(records, counts): counts (n,) uint32, the full numbers of neighbours.  With k > 0: records (n, k); with offsets ((n + 1,), taken
    as a host form takes them: starting at 0, not decreasing): records (offsets[-1],); with neither: the full lists and their CSR
    offsets, (offsets (n + 1,) int64, records, counts)."""
    q, d = np.asarray(points, F32).reshape(-1, 3), np.asarray(data, F32).reshape(-1, 3)
    n = len(q)
    r2 = bounds(n, radius2, max_dist2)
    counts = np.zeros(n, np.uint32)
    lists = []
    for b in range(0, n, block):
        e = min(n, b + block)
        mem, d2 = members(q[b:e], d, r2[b:e])
        if skip_same_index:
            for i in range(b, min(e, len(d))):
                mem[i - b, i] = False
        counts[b:e] = mem.sum(1)
        for i in range(e - b):
            j = np.flatnonzero(mem[i])
            j = j[np.argsort(d2[i, j], kind="stable")]  # (ascending j, then a stable sort by d2: ties go to the smaller index)
            rec = np.zeros(len(j), RECORD)
            rec["dist2"], rec["index"] = d2[i, j], j
            lists.append(rec)
    if k == 0 and offsets is None:
        off = np.zeros(n + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        return off, (np.concatenate(lists) if lists else np.zeros(0, RECORD)), counts
    off = np.arange(n + 1, dtype=np.int64) * k if offsets is None else np.asarray(offsets).astype(np.int64)
    out = np.zeros(int(off[-1]) if n else 0, RECORD)
    out["dist2"], out["index"] = np.inf, NO_PRIM
    for i, rec in enumerate(lists):
        s = min(len(rec), int(off[i + 1] - off[i]))
        out[off[i] : off[i] + s] = rec[:s]
    return (out.reshape(n, k) if offsets is None else out), counts


def first_k(offsets, records, k):
    """The k-record slots of the full lists (offsets, records): (n, k) records, the rest of a slot {+inf, NO_PRIM}."""
    n = len(offsets) - 1
    out = np.zeros((n, k), RECORD)
    out["dist2"], out["index"] = np.inf, NO_PRIM
    for i in range(n):
        s = min(k, int(offsets[i + 1] - offsets[i]))
        out[i, :s] = records[offsets[i] : offsets[i] + s]
    return out


def exact_d2(points, data):
    """(n, m) float64 from the float32 inputs: every step exact or correctly rounded in float64 (24-bit inputs: the differences are
    exact when the exponents are near, and in any case carry 2^-53 relative errors, nothing against the 2^-24 in question)."""
    q, d = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(data, np.float64).reshape(-1, 3)
    return ((q[:, None, :] - d[None, :, :]) ** 2).sum(-1)


def scale_cloud():
    """(data (4096, 3), queries (2048, 3)) of the across-scale tests: the uniform unit-cube cloud of test_point_neighbors_gpu._main()
    (seed 7), every eighth query set equal to a data point (256 of them)."""
    rng = np.random.default_rng(7)
    data, pts = rng.random((4096, 3)).astype(F32), rng.random((2048, 3)).astype(F32)
    pts[0::8] = data[0::16]
    return data, pts


def overflow_cloud(k=127, m=2048, n=512, seed=19):
    """(data (m, 3), queries (n, 3)): coordinates +-2^k * u, u uniform in [0.5, 1.99) -- at k = 127 all are finite, `x - lo` overflows to
    +inf for the part of the cloud more than 2^128 above the minimum, and d2 to +inf between all pairs that differ; every second query is
    a data point, and the first 64 data points are repeated at 64 .. 127 (exact duplicates)."""
    rng = np.random.default_rng(seed)
    with np.errstate(over="ignore"):
        u = rng.uniform(0.5, 1.99, (m + n, 3)) * rng.choice([-1.0, 1.0], (m + n, 3))
        p = np.ldexp(u.astype(F32), int(k)).astype(F32)
    data, pts = p[:m].copy(), p[m:].copy()
    data[64:128] = data[0:64]
    pts[0::2] = data[: n // 2]
    assert np.isfinite(p).all()
    return data, pts


def lattice_case():
    """An 8^3 lattice of spacing 0.25 (every coordinate and every distance exact)."""
    g = np.arange(8, dtype=F32) * F32(0.25)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)

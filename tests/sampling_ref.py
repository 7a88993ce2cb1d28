"""The surface sampler (include/cgrt.h "Surface sampling") restated in numpy from its definition -- not from the library's
sources.  Not a test module; numpy only.

  * Philox4x32-10 on uint64 arrays (a 32 x 32 product fits; the high and low words are a shift and a mask);
  * the areas by surface_ref.area (the reference's area function), what is NaN, infinite or not > 0 counted as 0;
  * the running sum by np.cumsum in float64 (sequential), the thresholds from it in float64;
  * the triangle by np.searchsorted(T[:L], x, side='right'); the integer fold of the two barycentric words; the float32 mix, every
    product and sum rounded once."""
import numpy as np

import surface_ref

F32 = np.float32
U64 = np.uint64
NO_PRIM = 0xFFFFFFFF
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = U64(0xFFFFFFFF)
S32 = U64(32)
SAMPLE_DTYPE = np.dtype([("point", F32, 3), ("mesh_id", np.uint32), ("prim_id", np.uint32), ("bary", F32, 3)])
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def philox4x32_10(counter, key):
    """counter: four uint32-valued arrays (or scalars), key: two -> the four output words as uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(x, U64)) & MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ U64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ U64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def philox_python(counter, key):
    """The same generator on Python integers (one counter), written apart from the array form."""
    c, k = [int(x) for x in counter], [int(x) for x in key]
    for _ in range(10):
        hi0, lo0 = divmod(0xD2511F53 * c[0], 1 << 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c[2], 1 << 32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + 0x9E3779B9) % (1 << 32), (k[1] + 0xBB67AE85) % (1 << 32)]
    return c


def vertices(sd):
    """(v0, v1, v2), each (ntris, 3) float32, in prim_id order."""
    pos = np.asarray(sd.pos_nrm, F32).reshape(-1, 6)[:, 0:3]
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    return [np.ascontiguousarray(pos[tri[:, k]]) for k in range(3)]


def areas(sd):
    """(ntris,) float32: the area of every triangle, 0 where it is NaN, infinite or not > 0."""
    v0, v1, v2 = vertices(sd)
    if len(v0) == 0:
        return np.zeros(0, F32)
    with np.errstate(**_ERR):
        a = surface_ref.area(v0, v1, v2)
        return np.where(np.isfinite(a) & (a > 0), a, F32(0)).astype(F32)


def table(sd):
    """(areas, total, thresholds (uint32), last): last is NO_PRIM when no triangle has an area (thresholds all 0 then)."""
    a = areas(sd)
    S = np.cumsum(a.astype(np.float64))
    pos = np.nonzero(a > 0)[0]
    if len(pos) == 0:
        return a, float(S[-1]) if len(S) else 0.0, np.zeros(len(a), np.uint32), NO_PRIM
    T = np.minimum(np.floor((S / S[-1]) * 4294967296.0), 4294967295.0).astype(np.uint32)
    return a, float(S[-1]), T, int(pos[-1])


def position_words(n, seed=0, first=0, strata=0):
    """(x, w1, w2) as uint64 arrays for samples first .. first + n - 1."""
    j = (np.arange(n, dtype=U64) + U64(first % (1 << 64)))
    seed = int(seed)
    w = philox4x32_10([j & MASK, j >> S32, 0, 0], [seed & 0xFFFFFFFF, seed >> 32])
    x = w[0]
    if strata:
        x = ((j << S32) | w[0]) // U64(strata)
    return x, w[1], w[2]


def weights(w1, w2):
    """The folded integer weights (c, a, b) of v0, v1, v2, each in 0 .. 2^24, summing to 2^24 (int64 arrays)."""
    a, b = (np.asarray(w1, U64) >> U64(8)).astype(np.int64), (np.asarray(w2, U64) >> U64(8)).astype(np.int64)
    fold = a + b > (1 << 24)
    a, b = np.where(fold, (1 << 24) - a, a), np.where(fold, (1 << 24) - b, b)
    return (1 << 24) - a - b, a, b


def sample(sd, n, seed=0, first=0, strata=0, attr=None, tab=None):
    """The n records (SAMPLE_DTYPE) and, with attr ((nverts, C) float32), the (n, C) rows -- (records, rows or None)."""
    _, _, T, last = table(sd) if tab is None else tab
    out = np.zeros(n, SAMPLE_DTYPE)
    if attr is not None:
        attr = np.asarray(attr, F32)
        attr = attr if attr.ndim == 2 else attr.reshape(len(attr), -1)
    rows = None if attr is None else np.zeros((n, attr.shape[1]), F32)
    if last == NO_PRIM:
        out["mesh_id"], out["prim_id"] = NO_PRIM, NO_PRIM
        return out, rows
    x, w1, w2 = position_words(n, seed, first, strata)
    prim = np.searchsorted(T[:last], x.astype(np.uint32), side="right").astype(np.int64)
    c, a, b = weights(w1, w2)
    bary = np.stack([c, a, b], 1).astype(F32) * F32(2.0 ** -24)
    v0, v1, v2 = vertices(sd)
    with np.errstate(**_ERR):
        out["point"] = (bary[:, 0:1] * v0[prim] + bary[:, 1:2] * v1[prim]) + bary[:, 2:3] * v2[prim]
    out["mesh_id"] = np.asarray(sd.tri_mesh, np.uint32)[prim]
    out["prim_id"] = prim
    out["bary"] = bary
    if attr is not None:
        t = attr
        tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[prim]
        with np.errstate(**_ERR):
            rows[:] = (bary[:, 0:1] * t[tri[:, 0]] + bary[:, 1:2] * t[tri[:, 1]]) + bary[:, 2:3] * t[tri[:, 2]]
    return out, rows


def points64(sd, rec):
    """The float64 mix of the records' own weights (exact integers over 2^24), and S = each triangle's largest |coordinate|."""
    prim = rec["prim_id"].astype(np.int64)
    v = [x[prim].astype(np.float64) for x in vertices(sd)]
    b = rec["bary"].astype(np.float64)
    p = b[:, 0:1] * v[0] + b[:, 1:2] * v[1] + b[:, 2:3] * v[2]
    return p, np.abs(np.concatenate(v, 1)).max(1)


def degenerate_scene(pkg):
    """Eight triangles on 24 vertices of their own: area 0 first, in the middle and last, one with a NaN vertex, one of about 2^-40 of the
    total area; two meshes."""
    big = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    e = 2.0 ** -20  # legs e: area e^2 / 2 = 2^-41, against a total of about 1.2
    T = [
        [[0, 0, 0], [1, 0, 0], [2, 0, 0]],            # 0: collinear
        big,                                           # 1
        [[0, 0, 1], [0.5, 0, 1], [0, 0.75, 1]],        # 2
        [[3, 3, 3], [3, 3, 3], [3, 3, 3]],             # 3: a point
        [[0, 0, 2], [float("nan"), 0, 2], [0, 1, 2]],  # 4: NaN
        [[5, 5, 5], [5 + e, 5, 5], [5, 5 + e, 5]],     # 5: tiny
        [[0, 0, 3], [1, 0, 3], [1, 1, 3]],             # 6
        [[1, 1, 1], [2, 2, 2], [1, 1, 1]],             # 7: collinear
    ]
    pos = np.asarray(T, F32).reshape(-1, 3)
    pn = np.concatenate([pos, np.tile(np.asarray([[0, 0, 1]], F32), (len(pos), 1))], 1).astype(F32)
    mats = np.tile(np.asarray([[0.5, 0.5, 0.5, 0, 0, 0, 1, 0]], F32), (2, 1))
    return pkg.scenes.SceneData(pos_nrm=pn, tri=np.arange(24, dtype=np.uint32).reshape(8, 3), tri_mesh=np.asarray([0, 0, 0, 0, 1, 1, 1, 1], np.uint32),
                                materials=mats, name="degenerate8")

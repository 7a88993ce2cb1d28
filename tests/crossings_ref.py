"""Ground truth of the crossing queries (include/cgrt.h "Crossing queries"), written from that text: the CPU oracle's
intersectRayWithTriangle (orc.ray_triangle) over ALL n x ntris pairs, each on a fresh copy of the ray, then the order (t as floats, -0
equal to +0; equal t to the smaller prim_id) and the slot rule.  Beside it the seeded ray families of the tests."""
import numpy as np

F32 = np.float32
NO_PRIM = 0xFFFFFFFF
FMAX = float(np.finfo(np.float32).max)
CROSSING_DTYPE = np.dtype([("t", np.float32), ("prim_id", np.uint32)])
FAMILIES = ("camera", "random", "at_vertices", "through_edges_and_vertices", "segments", "t_zero", "zero_component", "nan_inf")


def positions(sd):
    return np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3]


def tri18(sd):
    """(T, 18): v0 v1 v2 n1 n2 n3 of every triangle, prim_id order."""
    pn = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([pn[tri[:, k], 0:3] for k in range(3)] + [pn[tri[:, k], 3:6] for k in range(3)], axis=1))


def all_pairs(orc, sd, rays, chunk_pairs=1 << 20):
    """hit (n, T) bool and t (n, T) float32 of intersectRayWithTriangle on a fresh copy of ray i against triangle k."""
    r = np.ascontiguousarray(np.asarray(rays, np.float32).reshape(-1, 7))
    t18 = tri18(sd)
    T = len(t18)
    hit = np.zeros((len(r), T), bool)
    t = np.zeros((len(r), T), np.float32)
    step = max(1, chunk_pairs // max(T, 1))
    for s in range(0, len(r), step if T else len(r) + 1):
        c = r[s : s + step]
        res = orc.ray_triangle(np.tile(t18, (len(c), 1)), np.repeat(c, T, axis=0))
        hit[s : s + step] = (res["hit"] != 0).reshape(len(c), T)
        t[s : s + step] = res["t"].reshape(len(c), T)
    return hit, t


def crossings(hit, t):
    """counts (n,) uint32, offsets (n + 1,) int64 and the full list (CROSSING_DTYPE, ray after ray, each in order)."""
    ray, prim = np.nonzero(hit)
    tv = t[ray, prim]
    order = np.lexsort((prim, tv + F32(0.0), ray))  # (-0 + 0 = +0: the two zeros compare equal)
    rec = np.zeros(len(order), CROSSING_DTYPE)
    rec["t"], rec["prim_id"] = tv[order], prim[order]
    counts = hit.sum(axis=1).astype(np.uint32)
    offsets = np.zeros(len(hit) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return counts, offsets, rec


def reference(orc, sd, rays):
    return crossings(*all_pairs(orc, sd, rays))


def unused(n):
    out = np.zeros(n, CROSSING_DTYPE)
    out["t"], out["prim_id"] = np.inf, NO_PRIM
    return out


def slotted(ref, slots):
    """What a list call leaves in slots given as (n + 1,) boundaries: ray i's first min(size, count) crossings, then {+inf, NO_PRIM}."""
    counts, offsets, rec = ref
    slots = np.asarray(slots, np.int64)
    out = unused(int(slots[-1]))
    for i in range(len(counts)):
        m = min(int(slots[i + 1] - slots[i]), int(counts[i]))
        out[slots[i] : slots[i] + m] = rec[offsets[i] : offsets[i] + m]
    return out


def first_k(ref, k):
    n = len(ref[0])
    return slotted(ref, np.arange(n + 1, dtype=np.int64) * k).reshape(n, k)


def same_records(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == CROSSING_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- ray families ----
def _rays(o, d, t=FMAX):
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    r = np.zeros((len(o), 7), np.float32)
    r[:, 0:3], r[:, 3:6], r[:, 6] = o, d, t
    return r


def grown_box(sd, grow=0.25, pad=0.1):
    p = positions(sd)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    ext = hi - lo
    return lo - grow * ext - pad, hi + grow * ext + pad


def camera_rays(pkg, orc, m):
    """m rays of the default camera's 32 x 32 frame, evenly picked."""
    r = orc.generate_rays(pkg.scenes.default_camera(32, 32), 32, 32)
    return r[np.linspace(0, len(r) - 1, m).astype(np.int64)] if m < len(r) else r


def random_rays(sd, m, seed):
    rng = np.random.default_rng(seed)
    lo, hi = grown_box(sd)
    return _rays(rng.uniform(lo, hi, (m, 3)), rng.normal(size=(m, 3)))


def vertex_origin_rays(sd, m, seed):
    """Origins exactly at vertices: on the plane of every triangle that shares the vertex (and of every coplanar one)."""
    rng = np.random.default_rng(seed)
    p = positions(sd)
    return _rays(p[rng.integers(0, len(p), m)], rng.normal(size=(m, 3)))


def edge_and_vertex_rays(sd, m, seed):
    """Rays aimed at edge midpoints (even rows) and vertices (odd rows), unnormalised: t ~ 1 at the target, equal-t pairs on shared edges."""
    rng = np.random.default_rng(seed)
    p = positions(sd)
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    k, e = rng.integers(0, len(tri), m), rng.integers(0, 3, m)
    a, b = p[tri[k, e]], p[tri[k, (e + 1) % 3]]
    target = ((a + b) * F32(0.5)).astype(np.float32)
    target[1::2] = a[1::2]
    lo, hi = grown_box(sd)
    o = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    return _rays(o, target - o)


def segment_rays(orc, sd, m, seed):
    """Segments whose t is bit for bit the t of one of the ray's own crossings (the strict `<` of `t >= ray.t`)."""
    r = np.concatenate([random_rays(sd, m - m // 2, seed), edge_and_vertex_rays(sd, m // 2, seed + 1)])
    counts, offsets, rec = reference(orc, sd, r)
    rng = np.random.default_rng(seed + 2)
    for i in np.flatnonzero(counts):
        r[i, 6] = rec["t"][offsets[i] + rng.integers(0, counts[i])]
    return r


def t_zero_rays(sd, m, seed):
    r = np.concatenate([random_rays(sd, m - m // 2, seed), vertex_origin_rays(sd, m // 2, seed + 1)])
    r[:, 6] = 0.0
    return r


def zero_component_rays(sd, m, seed):
    r = random_rays(sd, m, seed)
    r[np.arange(m), 3 + np.arange(m) % 3] = 0.0
    idx = np.arange(m)[1::4]
    r[idx, 3 + (idx + 1) % 3] = -0.0
    return r


def nan_inf_rays():
    r = _rays([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3]], [[0.3, -0.5, 0.8], [0.3, -0.5, 0.8]])
    r[0, 1] = np.nan
    r[1, 4] = np.inf
    return r


def families(pkg, orc, sd, seed, camera=1024, random=512, other=64):
    """name -> rays (k, 7): the eight families."""
    return {
        "camera": camera_rays(pkg, orc, camera),
        "random": random_rays(sd, random, seed),
        "at_vertices": vertex_origin_rays(sd, other, seed + 10),
        "through_edges_and_vertices": edge_and_vertex_rays(sd, other, seed + 20),
        "segments": segment_rays(orc, sd, other, seed + 30),
        "t_zero": t_zero_rays(sd, other, seed + 40),
        "zero_component": zero_component_rays(sd, other, seed + 50),
        "nan_inf": nan_inf_rays(),
    }


def mixed_rays(pkg, orc, sd, n, seed):
    """n rays with the families interleaved (ray i is of family i % 7; the NaN and the inf ray at positions 5 and 40 where n allows), so that
    every prefix holds all of them."""
    m = (n + 6) // 7
    f = families(pkg, orc, sd, seed, camera=m, random=m, other=m)
    r = np.zeros((7 * m, 7), np.float32)
    for j, name in enumerate(FAMILIES[:7]):
        r[j::7] = f[name]
    r = r[:n].copy()
    for pos, special in zip((5, 40), f["nan_inf"]):
        if pos < n:
            r[pos] = special
    return r

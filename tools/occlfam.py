"""Occlusion rays for the shadow-verdict tests (tests/test_occlusion_gpu.py, tools/fuzz_shade.py): point-light shadow rays as the
frame spawns them (spawn_rays.h, main.cpp:104-111), the reference's verdict for them, and the ray families where a verdict is fragile.

The reference decides `hit && !(ray.t + 0.001f >= |fromPosToLight|)` from its CLOSEST hit (main.cpp:115-119).  The library's shadow
kernels answer the same question with a bounded any-hit search (walk_fast.h WALK_OCCLUDED), so their t need not be the closest one:
only the verdict is compared.  Everything here is float32 arithmetic in the reference's expression order."""
import numpy as np

FMAX = np.finfo(np.float32).max
EPS = np.float32(0.001)


def verdict(hit, t, dist):
    """main.cpp:115-119 in float32: in shadow iff the ray hit and !(t + 0.001f >= dist)."""
    t = np.asarray(t, np.float32)
    dist = np.asarray(dist, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(hit) != 0) & ~((t + EPS) >= dist)


def reference(o, rays, dist, threads=16):
    """The oracle's verdict: its closest hit (OracleScene.intersect, the rays' own t -- FLT_MAX as spawned) through verdict()."""
    ref = o.intersect(rays, threads=threads)
    return verdict(ref["hit"], ref["t"], dist), ref


def _dot(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        return (p[..., 0] + p[..., 1]) + p[..., 2]


def normalize(v):
    """glm::normalize(v) = v * (1.0f / sqrt(dot(v, v))) (cgrt_math.h)."""
    v = np.asarray(v, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v * (np.float32(1.0) / np.sqrt(_dot(v, v)))[..., None]


def length(v):
    v = np.asarray(v, np.float32)
    return np.sqrt(_dot(v, v))


def spawn(points, lights):
    """Shadow rays from every point towards every light position (spawn_rays.h spawn_shadow_ray): points (P, 3), lights (L, 3) ->
    rays (P * L, 7) with ray p * L + l, and dist (P * L,).  A light AT the point gives the zero vector's NaN direction and dist 0."""
    p = np.asarray(points, np.float32)[:, None, :]
    lp = np.asarray(lights, np.float32)[None, :, :]
    to = lp - p
    d = normalize(to)
    with np.errstate(invalid="ignore"):
        o = p + EPS * d
    n = p.shape[0] * lp.shape[1]
    rays = np.empty((n, 7), np.float32)
    rays[:, 0:3] = np.broadcast_to(o, to.shape).reshape(-1, 3)
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = FMAX
    return rays, length(to).reshape(-1)


def hit_points(o, rays, threads=16):
    """Closest hits of `rays` on the oracle: (pointOn = o + d * t, normal, the hit records) for the rays that hit."""
    r = np.ascontiguousarray(rays, np.float32)
    ref = o.intersect(r, threads=threads)
    m = ref["hit"] == 1
    pts = r[m, 0:3] + r[m, 3:6] * ref["t"][m][:, None]
    return pts.astype(np.float32), ref["normal"][m].astype(np.float32), ref[m]


def aimed_rays(sd, n, rng, origin=None):
    """n rays from outside the scene (or from `origin`) aimed at random points of its triangles and spheres: most of them hit."""
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3]
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 5)
    pts = []
    if len(sd.tri):
        tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[rng.integers(0, sd.ntris, n)]
        w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
        pts.append((p[tri] * w[:, :, None]).sum(1))
    if len(sph):
        k = rng.integers(0, len(sph), n)
        u = normalize(rng.normal(size=(n, 3)).astype(np.float32))
        pts.append(sph[k, 0:3] + u * sph[k, 3:4])
    pts = np.concatenate(pts)[rng.permutation(n * len(pts))[:n]]
    lo, hi = pts.min(0), pts.max(0)
    c, ext = (lo + hi) / 2, np.maximum(hi - lo, np.float32(1e-30))
    if origin is None:
        org = c + normalize(rng.normal(size=(n, 3)).astype(np.float32)) * (np.float32(1.5) * ext.max())
    else:
        org = np.broadcast_to(np.asarray(origin, np.float32), (n, 3))
    r = np.empty((n, 7), np.float32)
    r[:, 0:3] = org
    r[:, 3:6] = normalize(pts - org)
    r[:, 6] = FMAX
    return r


def spawned(o, sd, base_rays, rng, extra_lights=(), nrandom=3, max_points=1500, threads=16):
    """Shadow rays of real hits: the closest hits of base_rays (camera or aimed rays), towards the scene's lights, `nrandom` random
    lights about the scene, `extra_lights` (e.g. inside a closed mesh), and per point a light behind its surface, a light on its surface
    (the point itself: zero direction, dist 0) and a light at another hit point (dist ~ the distance between two surface points)."""
    pts, nrm, _ = hit_points(o, base_rays, threads)
    if len(pts) > max_points:
        k = rng.choice(len(pts), max_points, replace=False)
        pts, nrm = pts[k], nrm[k]
    if len(pts) == 0:
        return np.zeros((0, 7), np.float32), np.zeros(0, np.float32)
    lo, hi = pts.min(0), pts.max(0)
    c, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, np.float32(1e-30))
    L = [np.asarray(sd.point_lights, np.float32).reshape(-1, 6)[:, :3], np.asarray(extra_lights, np.float32).reshape(-1, 3),
         (c + rng.uniform(-1.6, 1.6, (nrandom, 3)) * ext).astype(np.float32)]
    rays, dist = spawn(pts, np.concatenate(L))
    out_r, out_d = [rays], [dist]
    # per point: behind its own surface, on it, and at another point of the surface
    behind = (pts - nrm * (np.float32(0.25) * ext.max())).astype(np.float32)
    other = pts[rng.permutation(len(pts))]
    for lp in (behind, pts, other):
        to = lp - pts
        d = normalize(to)
        with np.errstate(invalid="ignore"):
            org = pts + EPS * d
        r = np.concatenate([org, d, np.full((len(pts), 1), FMAX, np.float32)], 1).astype(np.float32)
        out_r.append(r)
        out_d.append(length(to))
    return np.concatenate(out_r), np.concatenate(out_d)


def ulps(x, k):
    """x moved by k float32 ulps (k may be negative)."""
    x = np.asarray(x, np.float32).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf) if k > 0 else np.float32(-np.inf)).astype(np.float32)
    return x


def boundary(o, rays, threads=16, max_rays=1500, rng=None):
    """The epsilon boundary: for rays that hit (closest t1), dist = fl(t1 + 0.001f) and its neighbours within +-2 ulps -- the verdict
    flips there -- and, along rays that hit a second layer behind the first (t2, found by casting again from just past t1), dist placed
    between the two layers' thresholds and at the second threshold +-1 ulp."""
    r = np.ascontiguousarray(rays, np.float32)
    ref = o.intersect(r, threads=threads)
    r = r[ref["hit"] == 1]
    t1 = ref["t"][ref["hit"] == 1]
    if rng is not None and len(r) > max_rays:
        k = rng.choice(len(r), max_rays, replace=False)
        r, t1 = r[k], t1[k]
    if len(r) == 0:
        return np.zeros((0, 7), np.float32), np.zeros(0, np.float32)
    th1 = (t1 + EPS).astype(np.float32)
    out_r, out_d = [], []
    for k in (-2, -1, 0, 1, 2):
        out_r.append(r)
        out_d.append(ulps(th1, k))
    # second layer: from just past the first hit, same direction
    step = np.maximum(np.abs(t1) * np.float32(1e-5), np.float32(1e-6)).astype(np.float32)
    r2 = r.copy()
    r2[:, 0:3] = r[:, 0:3] + r[:, 3:6] * (t1 + step)[:, None]
    ref2 = o.intersect(r2, threads=threads)
    m = ref2["hit"] == 1
    if m.any():
        t2 = (t1[m] + step[m] + ref2["t"][m]).astype(np.float32)
        th2 = (t2 + EPS).astype(np.float32)
        for dd in ((th1[m] + (th2 - th1[m]) * np.float32(0.5)).astype(np.float32), ulps(th2, -1), th2, ulps(th2, 1)):
            out_r.append(r[m])
            out_d.append(dd)
    return np.concatenate(out_r), np.concatenate(out_d).astype(np.float32)


def nonfinite(rays, dist):
    """Non-finite and degenerate inputs on top of real shadow rays: dist NaN, +inf, -inf, 0, -0, the smallest denormal; zero and NaN
    directions (a light at pointOn)."""
    r = np.ascontiguousarray(rays, np.float32)[:64]
    n = len(r)
    out_r, out_d = [], []
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, FMAX):
        out_r.append(r)
        out_d.append(np.full(n, v, np.float32))
    for d in ((0.0, 0.0, 0.0), (np.nan, np.nan, np.nan), (0.0, 0.0, 1e-45)):
        z = r.copy()
        z[:, 3:6] = d
        out_r.append(z)
        out_d.append(np.asarray(dist, np.float32)[:n])
    return np.concatenate(out_r), np.concatenate(out_d).astype(np.float32)


def scaled(sd, s, pkg):
    """The scene with every position multiplied by s (a power of two: exact), lights and spheres too."""
    pn = np.asarray(sd.pos_nrm, np.float32).copy()
    pn[:, :3] *= np.float32(s)
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 5).copy()
    sph[:, :4] *= np.float32(s)
    pl = np.asarray(sd.point_lights, np.float32).reshape(-1, 6).copy()
    pl[:, :3] *= np.float32(s)
    return pkg.scenes.SceneData(pos_nrm=pn, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials, spheres=sph, point_lights=pl)


def plates(pkg, n=12, gap=0.01):
    """n stacked square plates (two triangles each) at z = 0, gap, 2 gap, ...: rays along z cross every layer."""
    pos = []
    tri = []
    for k in range(n):
        z = np.float32(k * gap)
        b = len(pos)
        pos += [(-1, -1, z), (1, -1, z), (1, 1, z), (-1, 1, z)]
        tri += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
    pos = np.asarray(pos, np.float32)
    pn = np.concatenate([pos, np.tile(np.float32([0, 0, 1]), (len(pos), 1))], 1).astype(np.float32)
    tri = np.asarray(tri, np.uint32)
    mats = np.tile(np.float32([0.5, 0.5, 0.5, 0, 0, 0, 10, 1]), (1, 1))
    return pkg.scenes.SceneData(pos_nrm=pn, tri=tri, tri_mesh=np.zeros(len(tri), np.uint32), materials=mats,
                                point_lights=np.float32([[0.1, 0.2, 1.0, 1, 1, 1]]))


def duplicated(sd, pkg):
    """Every triangle twice in a row (same vertices, same mesh; meshes stay in order): closest hits tie."""
    tri = np.asarray(sd.tri, np.uint32).reshape(-1, 3)
    tm = np.asarray(sd.tri_mesh, np.uint32)
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=np.repeat(tri, 2, axis=0), tri_mesh=np.repeat(tm, 2), materials=sd.materials,
                                spheres=sd.spheres, point_lights=sd.point_lights)


def on_walls(sd, n, rng):
    """Origins exactly on the scene's axis-aligned triangles (the plane coordinate copied from a vertex), aimed into the scene, along
    the wall (a direction parallel to the face) and away from it; dist random up to the scene size."""
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3]
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    A, B, C = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    axis = -np.ones(len(tri), np.int64)
    for a in range(3):
        axis[(A[:, a] == B[:, a]) & (A[:, a] == C[:, a])] = a
    k = np.nonzero(axis >= 0)[0]
    if len(k) == 0:
        return np.zeros((0, 7), np.float32), np.zeros(0, np.float32)
    k = k[rng.integers(0, len(k), n)]
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    org = (A[k] * w[:, 0:1] + B[k] * w[:, 1:2] + C[k] * w[:, 2:3]).astype(np.float32)
    ax = axis[k]
    org[np.arange(n), ax] = A[k, ax]  # exactly on the plane
    lo, hi = p.min(0), p.max(0)
    c = (lo + hi) / 2
    d = normalize(c - org + rng.normal(scale=0.2, size=(n, 3)).astype(np.float32))
    par = d.copy()
    par[np.arange(n), ax] = 0.0  # parallel to the wall
    par = normalize(par)
    away = -d
    r = np.concatenate([np.concatenate([org, x, np.full((n, 1), FMAX, np.float32)], 1) for x in (d, par, away)]).astype(np.float32)
    dist = rng.uniform(0.0, 2.0 * float((hi - lo).max()), len(r)).astype(np.float32)
    return r, dist

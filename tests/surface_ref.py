"""The reference's barycentric weights and its normal mix, restated in numpy from src/ray_tracing.cpp:13-21 (magnitude, area) and :94-97
(alpha, beta, gamma, the mix) -- not from the library's cgrt_math.h.  Not a test module; numpy only.

Arithmetic, as the C++ evaluates it with glm 0.9.9.8 scalar code on x86-64:
  * `ray.origin + ray.direction * ray.t`, `v1 - v0`, glm::cross, `alpha * n1 + beta * n2 + gamma * n3`: float32, every product and
    every sum or difference rounded once (numpy float32 array arithmetic does exactly that);
  * magnitude (:13-16): pow(a.x, 2) promotes to double -- the squares are exact there --, the sum (x^2 + y^2) + z^2 and the sqrt are
    double, and the `float` return type narrows the result;
  * area (:17-21): `magnitude(...) / 2.0f`, a float32 division; the three ratios (:94-96) are float32 divisions;
  * glm::normalize(v) = v * (1.0f / sqrt(dot(v, v))), dot = (x*x + y*y) + z*z in float32;
  * the facing flip (:99-106): `dot(plane.normal, -ray.direction) > 0`, plane.normal = normalize(cross(v1 - v0, v2 - v0)) (:74-82).
"""
import numpy as np

F32 = np.float32
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _cross(a, b):
    """glm::cross on float32 (n, 3) arrays: (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y)."""
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    bx, by, bz = b[:, 0], b[:, 1], b[:, 2]
    return np.stack([ay * bz - by * az, az * bx - bz * ax, ax * by - bx * ay], axis=1)


def _dot(a, b):
    p = a * b
    return (p[:, 0] + p[:, 1]) + p[:, 2]


def _normalize(v):
    return v * (F32(1.0) / np.sqrt(_dot(v, v)))[:, None]


def magnitude(a):
    """ray_tracing.cpp:13-16."""
    d = a.astype(np.float64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)


def area(v0, v1, v2):
    """ray_tracing.cpp:17-21."""
    return magnitude(_cross(v1 - v0, v2 - v0)) / F32(2.0)


def triangle_vertices(sd, prim):
    pn = np.asarray(sd.pos_nrm, F32).reshape(-1, 6)
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[prim]
    return tri, [np.ascontiguousarray(pn[tri[:, k], 0:3]) for k in range(3)], [np.ascontiguousarray(pn[tri[:, k], 3:6]) for k in range(3)]


def _rays(rays):
    r = np.ascontiguousarray(rays)
    if r.dtype.fields is not None:
        r = r.view(F32).reshape(-1, 7)
    r = np.asarray(r, F32).reshape(-1, 7)
    return np.ascontiguousarray(r[:, 0:3]), np.ascontiguousarray(r[:, 3:6])


def triangle_mask(sd, hit, prim):
    """The items the definition gives weights: a hit on a triangle."""
    return (np.asarray(hit) != 0) & (np.asarray(prim, np.uint32) < np.uint32(sd.ntris))


def weights(sd, rays, t, prim, hit):
    """(n, 3) float32 {alpha, beta, gamma} of ray_tracing.cpp:94-96 for the triangle hits, zeros elsewhere."""
    o, d = _rays(rays)
    t = np.asarray(t, F32).reshape(-1)
    m = triangle_mask(sd, hit, prim)
    out = np.zeros((len(o), 3), F32)
    if not m.any():
        return out
    with np.errstate(**_ERR):
        _, (v0, v1, v2), _ = triangle_vertices(sd, np.asarray(prim, np.int64)[m])
        p = o[m] + d[m] * t[m][:, None]
        a = area(v0, v1, v2)
        out[m, 0] = area(p, v1, v2) / a
        out[m, 1] = area(p, v0, v2) / a
        out[m, 2] = area(p, v0, v1) / a
    return out


def mix(sd, w, prim, hit, attr):
    """(n, C) float32: (alpha * attr[i0] + beta * attr[i1]) + gamma * attr[i2] (the sum order of :97) for the triangle hits, zeros
    elsewhere."""
    attr = np.asarray(attr, F32)
    attr = attr.reshape(len(attr), -1)
    m = triangle_mask(sd, hit, prim)
    out = np.zeros((len(w), attr.shape[1]), F32)
    if m.any():
        tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[np.asarray(prim, np.int64)[m]]
        wm = np.asarray(w, F32)[m]
        with np.errstate(**_ERR):
            out[m] = (wm[:, 0:1] * attr[tri[:, 0]] + wm[:, 1:2] * attr[tri[:, 1]]) + wm[:, 2:3] * attr[tri[:, 2]]
    return out


def finish_normal(mixed, facing):
    """glm::normalize of the mix, negated where the plane does not face the ray (:97-106)."""
    with np.errstate(**_ERR):
        n = _normalize(np.asarray(mixed, F32))
    return np.where(np.asarray(facing)[:, None], n, -n)


def facing(sd, rays, prim):
    """dot(plane.normal, -ray.direction) > 0 (:99) for triangle hits `prim`."""
    _, d = _rays(rays)
    _, (v0, v1, v2), _ = triangle_vertices(sd, np.asarray(prim, np.int64))
    with np.errstate(**_ERR):
        pn = _normalize(_cross(v1 - v0, v2 - v0))
        return _dot(pn, -d) > 0


def normal(sd, rays, t, prim):
    """hitInfo.normal (:94-106) of triangle hits: every entry of `prim` is a triangle."""
    prim = np.asarray(prim, np.int64)
    ones = np.ones(len(prim), np.uint32)
    w = weights(sd, rays, t, prim, ones)
    vn = np.asarray(sd.pos_nrm, F32).reshape(-1, 6)[:, 3:6]
    return finish_normal(mix(sd, w, prim, ones, vn), facing(sd, rays, prim))


def weights64(sd, rays, prim):
    """Float64 signed-area barycentrics of the float64 plane hit of triangle hits `prim`, and what the error bound of the float32 weights
    needs: (w64 (n, 3), scale = max(1, |p|inf), h_min = 2A / L_max, |cos| between ray and plane normal, distance to the nearest edge in
    barycentric units)."""
    o, d = (x.astype(np.float64) for x in _rays(rays))
    _, (v0, v1, v2), _ = triangle_vertices(sd, np.asarray(prim, np.int64))
    v0, v1, v2 = (v.astype(np.float64) for v in (v0, v1, v2))
    with np.errstate(**_ERR):
        n = np.cross(v1 - v0, v2 - v0)
        nn = (n * n).sum(1)
        t = ((v0 - o) * n).sum(1) / (d * n).sum(1)
        p = o + d * t[:, None]
        w = np.stack([(np.cross(v1 - p, v2 - p) * n).sum(1), (np.cross(v2 - p, v0 - p) * n).sum(1), (np.cross(v0 - p, v1 - p) * n).sum(1)], 1) / nn[:, None]
        lmax = np.sqrt(np.maximum.reduce([((v1 - v0) ** 2).sum(1), ((v2 - v1) ** 2).sum(1), ((v0 - v2) ** 2).sum(1)]))
        hmin = np.sqrt(nn) / lmax
        cos = np.abs((d * n).sum(1)) / (np.sqrt((d * d).sum(1)) * np.sqrt(nn))
        scale = np.maximum(1.0, np.abs(p).max(1))
    return w, scale, hmin, cos, np.abs(w).min(1)


def random_rays(sd, n, seed):
    """n seeded rays (n, 7) float32 aimed at the scene from outside it: origins on a sphere around the vertices' bounding box, targets
    uniform in the box, t = FLT_MAX."""
    g = np.random.default_rng(seed)
    pos = np.asarray(sd.pos_nrm, F32).reshape(-1, 6)[:, 0:3].astype(np.float64)
    lo, hi = (pos.min(0), pos.max(0)) if len(pos) else (-np.ones(3), np.ones(3))
    c, r = (lo + hi) / 2, max(float(np.linalg.norm(hi - lo)), 1e-3)
    u = g.standard_normal((n, 3))
    o = c + 1.5 * r * u / np.linalg.norm(u, axis=1, keepdims=True)
    d = lo + g.random((n, 3)) * (hi - lo) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.empty((n, 7), F32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, np.finfo(F32).max
    return rays

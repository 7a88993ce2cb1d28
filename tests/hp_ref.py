"""The float64 referee: a plain, slow ray tracer in numpy that the CPU oracle and the device entries are held against.
Not a test module; numpy only.  It imports neither the oracle nor the package and shares no expression with them:

  triangles  Moeller-Trumbore (the reference, the oracle and the kernels intersect the plane, then test three edges);
  spheres    the textbook quadratic, nearest root in [0, limit);
  boxes      slab intervals;
  camera     rotation matrices Rz Ry Rx (the reference goes through a quaternion);
  shading    the *behaviour* of getFinalColor (main.cpp:61-98, 104-135, 160-235, 241-295), vectorised per recursion level.

All of it runs in float64 on the float32 inputs converted exactly, brute force over every primitive, no tree.

Hit rule.  A primitive is hit at parameter t when 0 <= t < the ray's own t (ray_tracing.cpp:59, :65, :149, :193); the nearest
such t wins.  hitInfo.normal of a triangle is the barycentric mix of the vertex normals, unit length, negated when the geometric
normal (v1-v0)x(v2-v0) does not face the ray (ray_tracing.cpp:94-106); of a sphere the outward unit normal (:156), never flipped.
hitInfo.material is written by triangles only (bounding_volume_hierarchy.cpp:878-879 passes the same HitInfo on to the spheres),
so a sphere hit carries the material of the nearest triangle inside the ray's limit, or none (-1: the default Material,
mesh.h:17-23, kd read as 0).

Ambiguity classes.  float32 may legitimately decide a ray either way; such rays are flagged, counted per class and capped by the
tests, never silently dropped:
  a  a candidate's plane hit lies within 1e-5 (barycentric) of one of its edges, or a sphere's discriminant within 1e-5 of zero
     relative to b^2, at or before the nearest hit;
  b  grazing: |cos(d, n)| < 1e-3 at the nearest hit;
  c  the two nearest accepted hits are closer than 1e-5 relative;
  d  the nearest t within 1e-5 relative of the ray's limit or of 0 (a sphere root within 1e-5 of 0 counts);
  e  the origin within 1e-6 (relative to coordinate magnitude) of some triangle's plane: the reference accepts such an origin at
     t = 0 when dot(o, n) == D exactly (ray_tracing.cpp:43-47), whatever the direction;
  f  non-finite or denormal inputs, a zero direction, a NaN limit;
  g  (shading) a diffuse or specular cosine within 1e-5 of its `<= 0` cut-off, a shadow verdict within 1e-5 relative of the
     distance rule, ks.z within 1e-6 of 0.01, or a flagged ray anywhere in the pixel's ray tree.

Error bound of t (u = 2^-24).  The reference evaluates, in float32, e1 = v1-v0, e2 = v2-v0, n = normalize(e1 x e2), D = v0.n,
den = d.n, num = D - o.n, t = num/den (ray_tracing.cpp:74-82, :50-58).  t does not depend on the length of n, so the roundings
of normalize's scale (dot, sqrt, reciprocal) cancel; what remains:
  * edges: one rounding per component.  Cross product: two products (3u each with the edge errors), one subtraction (u): every
    component is off by <= 4u (|ab| + |cd|), the vector by <= 4 sqrt(2) u |e1||e2| < 6u |e1||e2|, i.e. a *direction* error of n of
    6u s with the sliver factor s = |e1||e2| / |e1 x e2|, plus sqrt(3) u < 2u from normalize's final component-wise multiply:
    |eps| <= (6s + 2) u.
  * D and o.n: three products and two additions each, <= 3u |v0| and <= 3u |o|; the subtraction adds u |num|.  The tilted normal
    moves num by <= |v0 - o| |eps|.  Relative to |num| = |(v0-o).n|: u [(5 + 6s) (|v0| + |o|) / |num| + 1].
  * den: <= 3u |d| from the dot product, |d||eps| from the tilt: u (5 + 6s) |d| / |den|.
  * the division: u.
  Sum: u [(5 + 6s)(A + B) + 2] with A = (|v0| + |o|) / |(v0-o).n|, B = |d| / |d.n|.  As 5 + 6s <= 6 (1 + s) and
  cond = (A + B)(1 + s) >= 2, this is <= 7 u cond; K_T = 8 leaves one unit for the second-order terms.
      |t32 - t64| / t64 <= K_T * 2^-24 * cond,   cond = ((|v0| + |o|) / |(v0-o).n| + |d| / |d.n|) * (1 + |e1||e2| / |e1 x e2|)
  The oracle was measured at 0.17 - 0.69 of 2^-24 cond, so K_T = 8 is about twelve times the largest error seen: no inflation
  was needed, the derivation itself has that room (worst-case signs in every dot product).

Error bound of the normal (angle, radians).  The hit point p = o + d t is off by dp <= 4u (|o| + |d| t) + rel_t |d| t.  A
barycentric weight has gradient <= L / 2A (L the longest edge, A the area); the reference takes it as a ratio of two areas
(ray_tracing.cpp:94-96), each a cross product with <= 6u L^2 of error: dw <= (dp L + 6u L^2) / 2A + 3u.  The unnormalised mix m
moves by <= 3 dw max|n_i|, the angle by that over |m|, and normalize adds 4u:
      angle <= 4u + 3 max|n_i| / |m| * ((dp L + 6u L^2) / 2A + 3u)
A sphere's normal is normalize(p - c): angle <= 4u + 2 (dp + u |p|) / r.

Sphere.  b = 2 d.co, c = co.co - r^2, disc = b^2 - 4ac in float32, roots in double (ray_tracing.cpp:120-134): co carries u/2 per
component, b <= 4u |d||co|, c <= 4u (|co|^2 + r^2), disc <= 3u b^2 + 4a dc + 3u |4ac|; the root moves by (db + ddisc / (2 sqrt(disc)))
/ 2a.  With h = b / 2, so that sqrt(disc) = 2 sqrt(h^2 - ac), and K_S = 8 for the constants above:
      |dt| / t <= K_S u cond_s,   cond_s = (|d||co| + (h^2 + a (|co|^2 + r^2)) / sqrt(h^2 - ac)) / (a t)
Box.  (bound - o) / d is a subtraction and a division of exact inputs: every slab parameter, hence t, is within 2u (1 + u)
relative: K_B = 2.01, condition number 1.
"""
import numpy as np

U = 2.0 ** -24
K_T = 8.0
K_S = 8.0
K_B = 2.01
K_CAM = 32.0  # roundings between the camera's fields and a primary ray's direction, see camera_rays
FLT_MAX = float(np.finfo(np.float32).max)
FLT_TINY = float(np.finfo(np.float32).tiny)
BAND = 1e-5
GRAZE = 1e-3
ONPLANE = 1e-6
CLASSES = "abcdef"

_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def _len(v):
    with np.errstate(**_ERR):
        return np.sqrt((v * v).sum(-1))


def _unit(v):
    with np.errstate(**_ERR):
        return v / _len(v)[..., None]


def _dot(a, b):
    with np.errstate(**_ERR):
        return (a * b).sum(-1)


class Referee:
    def __init__(self, sd):
        pn = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6).astype(np.float64)
        tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
        self.T = len(tri)
        self.A, self.B, self.C = (pn[tri[:, k], :3] for k in range(3))
        self.NA, self.NB, self.NC = (pn[tri[:, k], 3:] for k in range(3))
        self.E1, self.E2 = self.B - self.A, self.C - self.A
        cr = np.cross(self.E1, self.E2) if self.T else np.zeros((0, 3))
        self.area2 = _len(cr)
        self.gn = _unit(cr)
        with np.errstate(**_ERR):
            self.sliver = _len(self.E1) * _len(self.E2) / self.area2
        self.longest = np.maximum(np.maximum(_len(self.E1), _len(self.E2)), _len(self.C - self.B)) if self.T else np.zeros(0)
        self.amax = np.abs(self.A).max(-1) if self.T else np.zeros(0)
        self.nmax = np.maximum(np.maximum(_len(self.NA), _len(self.NB)), _len(self.NC)) if self.T else np.zeros(0)
        self.tri_mesh = np.asarray(sd.tri_mesh, np.int64).reshape(-1)
        self.mats = np.asarray(sd.materials, np.float32).reshape(-1, 8).astype(np.float64)
        sp = np.asarray(sd.spheres, np.float32).reshape(-1, 5).astype(np.float64)
        self.SC, self.SR = sp[:, :3], sp[:, 3]
        self.S = len(sp)

    # ---------------------------------------------------------------------------------------------------------------------------
    def _triangles(self, o, d):
        """Moeller-Trumbore of n rays against all T triangles: t, u, v (n x T) and det."""
        A, E1, E2 = self.A, self.E1, self.E2
        ox, oy, oz = (o[:, k, None] for k in range(3))
        dx, dy, dz = (d[:, k, None] for k in range(3))
        e1x, e1y, e1z = (E1[None, :, k] for k in range(3))
        e2x, e2y, e2z = (E2[None, :, k] for k in range(3))
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x
        det = e1x * px + e1y * py + e1z * pz
        sx, sy, sz = ox - A[None, :, 0], oy - A[None, :, 1], oz - A[None, :, 2]
        with np.errstate(**_ERR):
            inv = 1.0 / det
            u = (sx * px + sy * py + sz * pz) * inv
            qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x
            v = (dx * qx + dy * qy + dz * qz) * inv
            t = (e2x * qx + e2y * qy + e2z * qz) * inv
        dist = np.abs(sx * self.gn[None, :, 0] + sy * self.gn[None, :, 1] + sz * self.gn[None, :, 2])
        return t, u, v, det, dist

    def _spheres(self, o, d):
        """Roots (n x S x 2, NaN where the line misses) of |o + t d - c| = r, the discriminant relative to b^2, and pieces of cond."""
        co = o[:, None, :] - self.SC[None]
        a = _dot(d, d)[:, None]
        hb = _dot(d[:, None, :], co)
        c = _dot(co, co) - self.SR[None] ** 2
        disc = hb * hb - a * c
        with np.errstate(**_ERR):
            sq = np.sqrt(disc)
            q = -(hb + np.copysign(sq, hb))  # the stable pair: q / a and c / q
            r0, r1 = q / a, c / q
            r1 = np.where(q == 0, r0, r1)
            roots = np.stack([np.minimum(r0, r1), np.maximum(r0, r1)], -1)
            rel = disc / (hb * hb + np.abs(a * c))
            cond_piece = (np.sqrt(a) * _len(co) + (hb * hb + a * (_dot(co, co) + self.SR[None] ** 2)) / sq) / a
        return roots, rel, cond_piece

    def nearest_hit(self, rays, chunk_elems=3_000_000):
        """rays: (n, 7) float32 {origin, direction, t}.  Returns a dict of per-ray arrays: hit, t, prim (triangle id, T + sphere index,
        -1), ngeo, normal, material, cond (t's condition number: rel error <= K * 2^-24 * cond, K_T or K_S by `sphere`), nbound (angle
        bound of the normal), sphere, flags (class -> bool), amb (any class)."""
        r = np.asarray(rays, np.float32).reshape(-1, 7)
        n = len(r)
        R = r.astype(np.float64)
        out = dict(hit=np.zeros(n, bool), t=np.full(n, np.inf), prim=np.full(n, -1, np.int64), ngeo=np.zeros((n, 3)),
                   normal=np.zeros((n, 3)), material=np.full(n, -1, np.int64), cond=np.zeros(n), nbound=np.zeros(n), sphere=np.zeros(n, bool))
        flags = {k: np.zeros(n, bool) for k in CLASSES}
        absr = np.abs(R[:, :6])
        flags["f"] = (~np.isfinite(R[:, :6]).all(1)) | ((absr > 0) & (absr < FLT_TINY)).any(1) | (R[:, 3:6] == 0).all(1) | np.isnan(R[:, 6])
        step = max(16, chunk_elems // max(self.T, 1))
        for s in range(0, n, step):
            self._nearest_chunk(np.nan_to_num(R[s:s + step], nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX), R[s:s + step, 6], slice(s, s + step), out, flags)
        out["flags"] = flags
        out["amb"] = np.logical_or.reduce([flags[k] for k in CLASSES])
        return out

    def _nearest_chunk(self, R, lim, sl, out, flags):
        o, d = R[:, :3], R[:, 3:6]
        n = len(R)
        rows = np.arange(n)
        dl = _len(d)
        best = np.full(n, np.inf)
        second = np.full(n, np.inf)
        tri_best = np.full(n, np.inf)
        ktri = np.zeros(n, np.int64)
        if self.T:
            t, u, v, det, dist = self._triangles(o, d)
            with np.errstate(**_ERR):
                w = 1.0 - u - v
            mb = np.minimum(np.minimum(u, v), w)
            ok = (det != 0) & (mb >= 0) & (t >= 0) & (t < lim[:, None])
            tt = np.where(ok, t, np.inf)
            ktri = tt.argmin(1)
            tri_best = tt[rows, ktri]
            tt[rows, ktri] = np.inf
            second = tt.min(1)
            best = tri_best.copy()
            flags["e"][sl] = (dist <= ONPLANE * np.maximum(np.abs(o).max(-1)[:, None], self.amax[None])).any(1)
        sph_best = np.full(n, np.inf)
        ksph = np.zeros(n, np.int64)
        near_zero_root = np.zeros(n, bool)
        if self.S:
            roots, rel, cpiece = self._spheres(o, d)
            okr = (roots >= 0) & (roots < lim[:, None, None])
            cand = np.where(okr, roots, np.inf).min(-1)  # nearest admissible root of each sphere
            ksph = cand.argmin(1)
            sph_best = cand[rows, ksph]
            cc = cand.copy()
            cc[rows, ksph] = np.inf
            four = np.sort(np.stack([tri_best, second, sph_best, cc.min(1)], 1), 1)  # the two nearest of each kind hold the two nearest
            best, second = four[:, 0], four[:, 1]
            scale = np.maximum(_len(o[:, None, :] - self.SC[None]), self.SR[None]) / np.maximum(dl, 1e-300)[:, None]
            near_zero_root = (np.abs(roots) < BAND * scale[..., None]).any((1, 2))
        hit = np.isfinite(best)
        is_s = hit & (sph_best < tri_best)
        slack = np.where(hit, best, np.inf) * (1 + BAND) + BAND
        lslack = lim * (1 + BAND) + BAND
        a = np.zeros(n, bool)
        if self.T:
            a |= ((np.abs(mb) < BAND) & (det != 0) & (t >= -BAND) & (t <= slack[:, None]) & (t < lslack[:, None])).any(1)
        if self.S:
            a |= ((np.abs(rel) < BAND) & ((roots[..., 0] <= slack[:, None]) | ~np.isfinite(roots[..., 0]))).any(1)
        flags["a"][sl] = a
        # the hit record
        p = o + d * np.where(hit, best, 0.0)[:, None]
        ng = np.zeros((n, 3))
        nrm = np.zeros((n, 3))
        cond = np.zeros(n)
        nb = np.zeros(n)
        with np.errstate(**_ERR):
            if self.T:
                k = ktri
                g = self.gn[k]
                uu, vv = u[rows, k], v[rows, k]
                m = (1.0 - uu - vv)[:, None] * self.NA[k] + uu[:, None] * self.NB[k] + vv[:, None] * self.NC[k]
                facing = _dot(g, d) < 0
                ni = _unit(m) * np.where(facing, 1.0, -1.0)[:, None]
                num = np.abs(_dot(self.A[k] - o, g))
                den = np.abs(_dot(d, g))
                ct = ((_len(self.A[k]) + _len(o)) / num + dl / den) * (1.0 + self.sliver[k])
                dp = 4 * U * (_len(o) + dl * best) + K_T * U * ct * dl * best
                L, A2 = self.longest[k], self.area2[k]
                nbt = 4 * U + 3 * self.nmax[k] / _len(m) * ((dp * L + 6 * U * L * L) / A2 + 3 * U)
                tri_hit = hit & ~is_s
                ng[tri_hit], nrm[tri_hit], cond[tri_hit], nb[tri_hit] = g[tri_hit], ni[tri_hit], ct[tri_hit], nbt[tri_hit]
            if self.S:
                k = ksph
                ns = _unit(p - self.SC[k])
                cs = cpiece[rows, k] / best
                dp = 4 * U * (_len(o) + dl * best) + K_S * U * cs * dl * best
                nbs = 4 * U + 2 * (dp + U * _len(p)) / self.SR[k]
                ng[is_s], nrm[is_s], cond[is_s], nb[is_s] = ns[is_s], ns[is_s], cs[is_s], nbs[is_s]
            cosn = np.abs(_dot(ng, d)) / dl
        flags["b"][sl] = hit & (cosn < GRAZE)
        with np.errstate(**_ERR):  # (a miss is inf - inf here)
            flags["c"][sl] = hit & (second - best < BAND * best)
            flags["d"][sl] = (hit & ((np.abs(best - lim) <= BAND * best) | (best <= BAND * (_len(o) + 1e-300) / np.maximum(dl, 1e-300)) | (best < BAND))) | near_zero_root
        out["hit"][sl], out["t"][sl] = hit, best
        out["prim"][sl] = np.where(hit, np.where(is_s, self.T + ksph, ktri), -1)
        out["ngeo"][sl], out["normal"][sl], out["cond"][sl], out["nbound"][sl], out["sphere"][sl] = ng, nrm, cond, nb, is_s
        if self.T:
            out["material"][sl] = np.where(hit & np.isfinite(tri_best), self.tri_mesh[ktri], -1)

    def any_hit(self, rays):
        """Occlusion of a segment: is anything hit at 0 <= t < the ray's own t.  Returns (occluded, ambiguous)."""
        h = self.nearest_hit(rays)
        f = h["flags"]
        return h["hit"], f["a"] | f["d"] | f["e"] | f["f"] | (h["hit"] & f["b"])

    # ---------------------------------------------------------------------------------------------------------------------------
    def shade(self, rays, lights, max_level):
        """getFinalColor of each ray under point lights (L x 6: position, colour), recursion as trace/shade (main.cpp:241-295) with `level
        >= max_level` in the place of `level >= 2`.  Returns rgb (n x 3 float64), unstable (class g, bool), and the per-class counts of
        the rays that made pixels unstable."""
        rays = np.asarray(rays, np.float32).reshape(-1, 7)
        lights = np.asarray(lights, np.float32).reshape(-1, 6).astype(np.float64)
        why = {}
        rgb, unstable = self._trace(0, rays[:, :3].astype(np.float64), rays[:, 3:6].astype(np.float64), rays[:, 6].astype(np.float64), lights,
                                    max_level, why)
        return rgb, unstable, why

    def _hit64(self, o, d, lim):
        """nearest_hit for float64 rays that the float32 drivers hold in float32: rounded the way they would be, to classify and to
        intersect the same ray."""
        with np.errstate(**_ERR):
            r = np.concatenate([o, d, lim[:, None]], 1).astype(np.float32)
        return self.nearest_hit(r), r.astype(np.float64)

    def point_in_shadow(self, P, light):
        """pointInShadow (main.cpp:104-135) of float64 points for one light: the ray starts 0.001 along the unit direction to the light
        with the float maximum as its limit; a hit shadows the point unless t + 0.001 >= |light - point|.  Returns the verdict, whether
        float32 may differ (the shadow ray is class a, d, e or f, or the verdict within 1e-5 relative of the distance rule), and the unit
        direction to the light."""
        eps = 0.001
        to = np.asarray(light, np.float64)[:3] - P
        dist = _len(to)
        tl = to / dist[:, None]
        sh, _ = self._hit64(P + eps * tl, tl, np.full(len(P), FLT_MAX))
        f = sh["flags"]
        near_rule = sh["hit"] & (np.abs(sh["t"] + eps - dist) < BAND * dist)
        return sh["hit"] & ~(sh["t"] + eps >= dist), f["a"] | f["d"] | f["e"] | f["f"] | near_rule, tl

    def _trace(self, level, o, d, lim, lights, max_level, why):
        n = len(o)
        rgb = np.zeros((n, 3))
        unstable = np.zeros(n, bool)
        if level >= max_level or n == 0:  # main.cpp:267-272
            return rgb, unstable
        h, R = self._hit64(o, d, lim)
        o, d = R[:, :3], R[:, 3:6]
        unstable |= h["amb"]
        for k in CLASSES:
            why[k] = why.get(k, 0) + int(h["flags"][k].sum())
        idx = np.nonzero(h["hit"])[0]  # a miss is black (:288-294)
        if len(idx) == 0:
            return rgb, unstable
        o, d, t, N = o[idx], d[idx], h["t"][idx], h["normal"][idx]
        mat = np.where((h["material"][idx] >= 0)[:, None], self.mats[np.maximum(h["material"][idx], 0)] if len(self.mats) else 0.0,
                       np.array([0, 0, 0, 0, 0, 0, 1.0, 1.0])[None])
        kd, ks, shin = mat[:, 0:3], mat[:, 3:6], mat[:, 6]
        P = o + d * t[:, None]  # :164
        refl = _unit(d - 2.0 * _dot(N, d)[:, None] * N)  # :64, :253
        col = np.zeros((len(idx), 3))
        uns = np.zeros(len(idx), bool)
        eps = 0.001
        for L in lights:  # :220-232
            shadow, samb, tl = self.point_in_shadow(P, L)
            cd = _dot(tl, N)  # :87-97
            cs = _dot(refl, tl)  # :69-78
            lit_d = (L[3:6] * kd).any(1)
            lit_s = (L[3:6] * ks).any(1)
            uns |= (samb & (lit_d | lit_s)) | (lit_d & (np.abs(cd) < BAND)) | (lit_s & (np.abs(cs) < BAND))
            with np.errstate(**_ERR):
                dif = np.where((cd > 0)[:, None], L[3:6] * kd * cd[:, None], 0.0)
                spe = np.where((cs > 0)[:, None], L[3:6] * ks * np.power(np.maximum(cs, 0.0), shin)[:, None], 0.0)
            col += np.where(shadow[:, None], 0.0, dif + spe)
        uns |= np.abs(ks[:, 2] - 0.01) < 1e-6
        why["g"] = why.get("g", 0) + int(uns.sum())
        mirror = np.nonzero(ks[:, 2] > 0.01)[0]  # :246, the comma operator leaves the last comparison
        if len(mirror):
            j = mirror
            rc, ru = self._trace(level + 1, P[j] + eps * refl[j], refl[j], _len(d[j]), lights, max_level, why)  # :254-260
            col[j] += rc * ks[j]  # :263
            uns[j] |= ru
        rgb[idx] = col
        unstable[idx] |= uns
        return rgb, unstable


def nearest_hit(sd, rays):
    """Referee(sd).nearest_hit(rays); build the Referee once when a scene is asked more than one question."""
    return Referee(sd).nearest_hit(rays)


def any_hit(sd, rays):
    return Referee(sd).any_hit(rays)


def shade(sd, rays, lights, max_level):
    return Referee(sd).shade(rays, lights, max_level)


# -------------------------------------------------------------------------------------------------------------------------------
# Cameras
# -------------------------------------------------------------------------------------------------------------------------------
def camera_rays(cam, W, H, rect=None):
    """The Trackball camera (trackball.cpp:70-73, :92-103; main.cpp's pixel loop: ndc = p / size * 2 - 1) in float64.  cam: look_at(3)
    euler(3) distance fovy aspect.  glm::quat(euler) is the rotation Rz(e.z) Ry(e.y) Rx(e.x); it is applied here as matrices.
    Returns origins and unit directions, row-major over rect = (x0, y0, x1, y1).

    float32 roundings on the way to a direction: ndc 3, half sizes 2 (tan, product), products with ndc 2, normalize 4 (dot, sqrt,
    reciprocal, multiply), half angles and sin/cos 3, the quaternion's four components 3 each (counted once: they act together), v + 2
    (w (q x v) + q x (q x v)) about 12 on a unit vector: 29, K_CAM = 32.  Every one moves the unit direction by at most u, so the angle
    is within K_CAM * 2^-24; the origin, a rotated (0, 0, -distance) plus look_at, within K_CAM * 2^-24 * (distance + |look_at|)."""
    a = np.asarray(cam, np.float32).reshape(9).astype(np.float64)
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    ex, ey, ez = a[3:6]

    def rx(t):
        return np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])

    def ry(t):
        return np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])

    def rz(t):
        return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])

    Rm = rz(ez) @ ry(ey) @ rx(ex)
    ys, xs = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), indexing="ij")
    nx = 2.0 * xs.reshape(-1) / W - 1.0
    ny = 2.0 * ys.reshape(-1) / H - 1.0
    hh = np.tan(a[7] / 2.0)
    hw = a[8] * hh
    cs = _unit(np.stack([-nx * hw, ny * hh, np.ones_like(nx)], 1))
    dirs = cs @ Rm.T
    org = a[0:3] + Rm @ np.array([0.0, 0.0, -a[6]])
    return np.broadcast_to(org, dirs.shape).copy(), dirs


def raycam_rays(cam20, W, H, x0=0, y0=0, w=None, h=None):
    """The affine ray camera (include/cgrt.h CgrtRayCamera) in float64: origin and unnormalised direction affine in (x + x_off, y +
    y_off); the direction is returned unit.  cam20: the record's 20 float32 words (offsets by bit pattern)."""
    a = np.ascontiguousarray(cam20, np.float32).reshape(20)
    off = a[18:20].view(np.int32).astype(np.float64)
    f = a[:18].astype(np.float64)
    w = W - x0 if w is None else w
    h = H - y0 if h is None else h
    ys, xs = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    fx = (xs.reshape(-1) + off[0])[:, None]
    fy = (ys.reshape(-1) + off[1])[:, None]
    org = f[0:3] + fx * f[3:6] + fy * f[6:9]
    v = f[9:12] + fx * f[12:15] + fy * f[15:18]
    # abs error of the float32 evaluation, per component: two products, two additions
    oerr = 2 * U * (np.abs(f[0:3]) + np.abs(fx * f[3:6]) + np.abs(fy * f[6:9])).max(1)
    verr = 2 * U * (np.abs(f[9:12]) + np.abs(fx * f[12:15]) + np.abs(fy * f[15:18]))
    aerr = np.sqrt((verr ** 2).sum(1)) / _len(v) + 4 * U  # angle: the affine part, then normalize
    return org, _unit(v), oerr * np.sqrt(3.0), aerr


# -------------------------------------------------------------------------------------------------------------------------------
# Element-wise forms of the six primitives (ray_tracing.h:10-20), one input row per ray
# -------------------------------------------------------------------------------------------------------------------------------
def _rays64(rays):
    r = np.asarray(rays, np.float32).reshape(-1, 7).astype(np.float64)
    return r[:, :3], r[:, 3:6], r[:, 6]


def _bad_inputs(*arrs):
    bad = np.zeros(len(arrs[0]), bool)
    for x in arrs:
        x = np.abs(x.reshape(len(x), -1))
        bad |= (~np.isfinite(x)).any(1) | ((x > 0) & (x < 1e-12)).any(1) | (x > 1e12).any(1)  # products of two such leave float32's range
    return bad


def ray_triangle(tri18, rays):
    """Row i: triangle v0 v1 v2 n1 n2 n3 against ray i.  Returns hit, t, normal, margin (True: float32 may differ), rel bound of t, angle bound."""
    q = np.asarray(tri18, np.float32).reshape(-1, 18).astype(np.float64)
    o, d, lim = _rays64(rays)
    A, B, C = q[:, 0:3], q[:, 3:6], q[:, 6:9]
    e1, e2 = B - A, C - A
    with np.errstate(**_ERR):
        pv = np.cross(d, e2)
        det = _dot(e1, pv)
        s = o - A
        u = _dot(s, pv) / det
        qv = np.cross(s, e1)
        v = _dot(d, qv) / det
        t = _dot(e2, qv) / det
        w = 1 - u - v
        mb = np.minimum(np.minimum(u, v), w)
        hit = (det != 0) & (mb >= 0) & (t >= 0) & (t < lim)
        cr = np.cross(e1, e2)
        g = _unit(cr)
        m = w[:, None] * q[:, 9:12] + u[:, None] * q[:, 12:15] + v[:, None] * q[:, 15:18]
        nrm = _unit(m) * np.where(_dot(g, d) < 0, 1.0, -1.0)[:, None]
        dl = _len(d)
        sl = _len(e1) * _len(e2) / _len(cr)
        num, den = np.abs(_dot(A - o, g)), np.abs(_dot(d, g))
        cond = ((_len(A) + _len(o)) / num + dl / den) * (1 + sl)
        dp = 4 * U * (_len(o) + dl * np.abs(t)) + K_T * U * cond * dl * np.abs(t)
        L = np.maximum(np.maximum(_len(e1), _len(e2)), _len(C - B))
        nmax = np.maximum(np.maximum(_len(q[:, 9:12]), _len(q[:, 12:15])), _len(q[:, 15:18]))
        nb = 4 * U + 3 * nmax / _len(m) * ((dp * L + 6 * U * L * L) / _len(cr) + 3 * U)
        scale = np.maximum(np.abs(o).max(1), np.abs(A).max(1))
        margin = (np.abs(mb) < BAND) | (den / dl < GRAZE) | (np.abs(t - lim) <= BAND * np.abs(t)) | (np.abs(t) * dl <= BAND * (_len(o) + _len(A)))
        margin |= (num <= ONPLANE * scale) | _bad_inputs(q[:, :9], o, d) | ~np.isfinite(t) | (K_T * U * cond > 0.1)
    return hit, t, nrm, margin, K_T * U * cond, nb


def ray_plane(plane4, rays):
    """Row i: plane (D, normal) against ray i: t = (D - o.n) / (d.n), accepted when 0 <= t < limit.  Error: both dot products within
    3u of their absolute sums, one subtraction, one division: 4u * ((|o||n| + |D|) / |D - o.n| + |d||n| / |d.n|)."""
    q = np.asarray(plane4, np.float32).reshape(-1, 4).astype(np.float64)
    o, d, lim = _rays64(rays)
    D, nn = q[:, 0], q[:, 1:4]
    with np.errstate(**_ERR):
        num, den = D - _dot(o, nn), _dot(d, nn)
        t = num / den
        hit = (den != 0) & (t >= 0) & (t < lim)
        cond = (_len(o) * _len(nn) + np.abs(D)) / np.abs(num) + _len(d) * _len(nn) / np.abs(den)
        margin = (np.abs(num) <= 1e-5 * (_len(o) * _len(nn) + np.abs(D))) | (np.abs(den) < GRAZE * _len(d) * _len(nn))
        margin |= (np.abs(t - lim) <= BAND * np.abs(t)) | _bad_inputs(q, o, d) | ~np.isfinite(t) | (4 * U * cond > 0.1)
    return hit, t, margin, 4 * U * cond


def triangle_plane(tri9):
    """(D, unit normal) of v0 v1 v2 with the orientation (v1-v0) x (v2-v0).  Bounds: the normal's angle (6s + 2) u (module docstring),
    D within 3u |v0| + |v0| * angle."""
    q = np.asarray(tri9, np.float32).reshape(-1, 9).astype(np.float64)
    e1, e2 = q[:, 3:6] - q[:, 0:3], q[:, 6:9] - q[:, 0:3]
    with np.errstate(**_ERR):
        cr = np.cross(e1, e2)
        nn = _unit(cr)
        D = _dot(q[:, 0:3], nn)
        ang = (6 * _len(e1) * _len(e2) / _len(cr) + 2 + 4) * U  # + normalize's own 4u
        derr = _len(q[:, 0:3]) * (3 * U + ang) + U * np.abs(D)
        margin = _bad_inputs(q) | ~np.isfinite(nn).all(1) | (_len(cr) < 1e-30) | (ang > 0.1)
    return D, nn, margin, ang, derr


def point_in_triangle(in15):
    """Row: v0 v1 v2 n p.  Inside when p is on the inner side (with respect to n) of all three edges, the boundary included
    (ray_tracing.cpp:33).  Margin: some side value within 1e-5 of zero relative to |n||edge||p - v|."""
    q = np.asarray(in15, np.float32).reshape(-1, 15).astype(np.float64)
    v = [q[:, 0:3], q[:, 3:6], q[:, 6:9]]
    nn, p = q[:, 9:12], q[:, 12:15]
    inside = np.ones(len(q), bool)
    margin = _bad_inputs(q)
    for i in range(3):
        e, r = v[(i + 1) % 3] - v[i], p - v[i]
        s = _dot(nn, np.cross(e, r))
        inside &= s >= 0
        margin |= np.abs(s) <= BAND * _len(nn) * _len(e) * _len(r)
    return inside, margin


def ray_box(box6, rays):
    """Row i: box (lower, upper) against ray i by slab intervals.  Returns hit, t, starts-inside (strict: bvh.cpp:647-661), margin.
    t is the entry parameter, or the exit parameter when the entry lies behind the origin (ray_tracing.cpp:184-191)."""
    q = np.asarray(box6, np.float32).reshape(-1, 6).astype(np.float64)
    o, d, lim = _rays64(rays)
    lo, hi = q[:, 0:3], q[:, 3:6]
    with np.errstate(**_ERR):
        ta, tb = (lo - o) / d, (hi - o) / d
        near, far = np.minimum(ta, tb), np.maximum(ta, tb)
        tin, tout = near.max(1), far.min(1)
        hit0 = (tin <= tout) & (tout >= 0)
        t = np.where(tin < 0, tout, tin)
        hit = hit0 & (t < lim)
        inside = ((lo < o) & (o < hi)).all(1)
        # margin: a verdict decided by two different axes' parameters closer than 1e-5, by tout or tin against 0, by t against the limit
        scale = np.maximum(np.abs(near), np.abs(far)).max(1)
        cross = np.full(len(q), np.inf)
        for i in range(3):
            for j in range(3):
                if i != j:
                    cross = np.minimum(cross, np.abs(far[:, j] - near[:, i]))
        margin = (cross <= BAND * scale) | (np.abs(tout) <= BAND * scale) | (np.abs(tin) <= BAND * scale) | (np.abs(t - lim) <= BAND * np.abs(t))
        margin |= np.isnan(near).any(1) | np.isnan(far).any(1) | _bad_inputs(q, o, d) | ~np.isfinite(t)
        margin |= ((d == 0) & ((np.abs(o - lo) <= ONPLANE * scale[:, None]) | (np.abs(o - hi) <= ONPLANE * scale[:, None]))).any(1)
    return hit, t, inside, margin


def ray_sphere(sph4, rays):
    """Row i: sphere (centre, radius) against ray i: nearest root in [0, limit).  Returns hit, t, outward unit normal, margin, rel bound of t, angle bound."""
    q = np.asarray(sph4, np.float32).reshape(-1, 4).astype(np.float64)
    o, d, lim = _rays64(rays)
    co, r = o - q[:, 0:3], q[:, 3]
    with np.errstate(**_ERR):
        a, hb, c = _dot(d, d), _dot(d, co), _dot(co, co) - r * r
        disc = hb * hb - a * c
        sq = np.sqrt(disc)
        qq = -(hb + np.copysign(sq, hb))
        r0 = qq / a
        r1 = np.where(qq == 0, r0, c / qq)
        lo_, hi_ = np.minimum(r0, r1), np.maximum(r0, r1)
        t = np.where(lo_ >= 0, lo_, hi_)
        hit = (disc >= 0) & (t >= 0) & (t < lim)
        p = o + d * t[:, None]
        nrm = _unit(p - q[:, 0:3])
        dl = np.sqrt(a)
        cond = (dl * _len(co) + (hb * hb + a * (_dot(co, co) + r * r)) / sq) / (a * np.abs(t))
        dp = 4 * U * (_len(o) + dl * np.abs(t)) + K_S * U * cond * dl * np.abs(t)
        nb = 4 * U + 2 * (dp + U * _len(p)) / r
        rel = disc / (hb * hb + np.abs(a * c))
        scale = np.maximum(_len(co), r) / dl
        margin = (np.abs(rel) < BAND) | (np.abs(lo_) < BAND * scale) | (np.abs(hi_) < BAND * scale) | (np.abs(t - lim) <= BAND * np.abs(t))
        margin |= _bad_inputs(q, o, d) | (hit & ~np.isfinite(cond)) | (hit & (K_S * U * cond > 0.1))
    return hit, t, nrm, margin, K_S * U * cond, nb


def angle(a, b):
    """Angle between rows of unit-ish vectors, radians, stable near 0."""
    a, b = _unit(np.asarray(a, np.float64)), _unit(np.asarray(b, np.float64))
    return 2.0 * np.arcsin(np.minimum(1.0, 0.5 * _len(a - b)))

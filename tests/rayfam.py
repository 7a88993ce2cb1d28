"""Seeded ray families for parity tests: a primary grid plus adversarial rays --
axis-parallel directions (zero components => +-inf / NaN slabs), origins on box faces, inside boxes and on
triangle planes, finite ray.t (shadow style), edge- and vertex-grazing rays, and the three cube.obj rays on
which the reference's BVH misses a hit its brute force finds."""
import numpy as np

FMAX = np.finfo(np.float32).max
SEED = 0x5EEDC0DE  # recorded in every fixture header

F4_ORIGIN = (1.1, 1.3, -2.6)
F4_DIRS = [
    (-0.355097264, -0.411639154, 0.839320719),
    (-0.378721297, -0.235073969, 0.895159364),
    (-0.380845577, -0.211262539, 0.900180399),
]
# what the reference itself produced for them during the survey probe:
F4_BRUTE_T = ["3.09774303", "2.90451074", "2.88830972"]


def _mk(o, d, t=None):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    d = np.asarray(d, np.float32).reshape(-1, 3)
    n = max(len(o), len(d))
    r = np.zeros((n, 7), np.float32)
    r[:, 0:3] = o
    r[:, 3:6] = d
    r[:, 6] = FMAX if t is None else np.asarray(t, np.float32)
    return r


def _norm(v):
    v = np.asarray(v, np.float64)
    return (v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-30)).astype(np.float32)


def families(sd, node_boxes, primary, rng=None, n_random=1500):
    """sd: SceneData; node_boxes: (N,6) AABBs of the reference tree; primary: (P,7) camera rays.
    Returns dict name -> (n,7) float32 rays."""
    rng = np.random.RandomState(SEED & 0x7FFFFFFF) if rng is None else rng
    fam = {"primary": primary.astype(np.float32)}
    cam_pos = primary[0, 0:3] if len(primary) else np.array([1.0, 1.0, -2.5], np.float32)

    # random origins / directions, normalised and not
    o = rng.uniform(-2.0, 2.0, (n_random, 3))
    tgt = rng.uniform(-0.6, 0.6, (n_random, 3))
    d = tgt - o
    fam["random_unit"] = _mk(o, _norm(d))
    fam["random_scaled"] = _mk(o, (d * rng.uniform(0.05, 7.0, (n_random, 1))).astype(np.float32))
    # finite ray.t (shadow-style), incl. t shorter than the hit distance, zero and tiny
    tt = rng.uniform(0.0, 4.0, n_random).astype(np.float32)
    tt[:16] = [0.0, 1e-30, 1e-6, 1e-3, 0.5, 1.0, 2.0, 3.0, 1e10, FMAX, np.inf, 0.25, 0.75, 1.5, 2.5, 3.5]
    fam["finite_t"] = _mk(o, _norm(d), tt)

    V = sd.pos_nrm[:, 0:3]
    T = sd.tri
    if len(T):
        k = rng.randint(0, len(T), min(600, 40 * len(T)))
        A, B, C = V[T[k, 0]], V[T[k, 1]], V[T[k, 2]]
        # vertex- and edge-grazing from the camera position, and from random origins
        for name, P in (("graze_vertex", A), ("graze_edge", ((A.astype(np.float64) + B) / 2).astype(np.float32)),
                        ("graze_centroid", ((A.astype(np.float64) + B + C) / 3).astype(np.float32))):
            fam[name] = _mk(np.broadcast_to(cam_pos, P.shape), _norm(P - cam_pos))
        # origins ON triangle planes (vertex, edge midpoint, interior point) shooting along +-normal and sideways
        nrm = np.cross(B - A, C - A)
        w = rng.dirichlet((1, 1, 1), len(k)).astype(np.float32)
        inner = (w[:, 0:1] * A + w[:, 1:2] * B + w[:, 2:3] * C).astype(np.float32)
        oo = np.concatenate([A, ((A + B) * np.float32(0.5)).astype(np.float32), inner, inner])
        dd = np.concatenate([_norm(nrm), _norm(-nrm), _norm(nrm), _norm(B - A)])
        fam["on_plane"] = _mk(oo, dd)

    if len(node_boxes):
        bx = node_boxes[rng.randint(0, len(node_boxes), 400)]
        lo, hi = bx[:, 0:3], bx[:, 3:6]
        ctr = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
        axes = np.eye(3, dtype=np.float32)
        oo, dd = [], []
        for a in range(3):
            for sgn in (1.0, -1.0):
                # axis-parallel rays: from outside through the box centre, from ON the lower/upper face, from the centre
                dvec = axes[a] * np.float32(sgn)
                start = ctr.copy()
                start[:, a] = lo[:, a] - 1.5 if sgn > 0 else hi[:, a] + 1.5
                oo += [start, lo, hi, ctr]
                dd += [np.broadcast_to(dvec, ctr.shape)] * 4
                # two zero components and an origin exactly in a face plane but outside the face
                off = lo.copy()
                off[:, (a + 1) % 3] -= 0.25
                oo.append(off)
                dd.append(np.broadcast_to(dvec, ctr.shape))
        # one zero component (diagonal in a plane), origins at box corners / centres
        for a in range(3):
            dvec = np.ones(3, np.float32)
            dvec[a] = 0.0
            oo += [lo - np.float32(0.5) * dvec, ctr]
            dd += [np.broadcast_to(_norm(dvec), ctr.shape)] * 2
        fam["axis_parallel"] = _mk(np.concatenate(oo), np.concatenate(dd))
        # inside boxes with random directions, and negative-zero direction components
        dz = _norm(rng.normal(size=(len(ctr), 3)))
        dz[::3, 0] = -0.0
        dz[1::3, 1] = 0.0
        fam["inside_boxes"] = _mk(ctr, dz)

    # extreme magnitudes: far-away origins aimed at the scene, tiny / huge direction scales, mixed
    # (exercise the "irregular ray" fallback of the in-leaf accelerator and overflow/underflow paths)
    m = 240
    tgt2 = rng.uniform(-0.5, 0.5, (m, 3))
    dirs = _norm(rng.normal(size=(m, 3))).astype(np.float64)
    dist = np.repeat([1e3, 1e6, 1e9, 1e13, 3e-3, 30.0], m // 6)[:, None]
    oo = (tgt2 - dirs * dist).astype(np.float32)
    dd = dirs.astype(np.float32)
    scl = np.tile(np.float32([1.0, 1e-15, 1e15, 1e-30, 1e30, 1e-38]), m // 6)[:, None]
    fam["extreme"] = _mk(oo, (dd * scl).astype(np.float32))

    fam["f4_cube"] = _mk(np.broadcast_to(np.float32(F4_ORIGIN), (3, 3)), np.float32(F4_DIRS))
    return fam


def concat(fam):
    return np.concatenate([fam[k] for k in sorted(fam)]).astype(np.float32)


def arbitrary_rays(sd, n, seed):
    """Seeded rays about a scene's mesh bounds (written for the Cornell box): origins inside, outside and on its surfaces, directions of length 0.25..4, t either the
    float maximum, finite beyond the scene, or shorter than the first hit."""
    rng = np.random.default_rng(seed)
    p = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, :3]
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, (hi - lo) / 2
    o = np.empty((n, 3), np.float32)
    k = n // 3
    o[:k] = c + rng.uniform(-0.9, 0.9, (k, 3)) * ext  # inside
    o[k : 2 * k] = c + rng.uniform(-3.0, 3.0, (k, 3)) * ext  # mostly outside
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    pick = tri[rng.integers(0, len(tri), n - 2 * k)]  # on surfaces: random points of random triangles
    w = rng.dirichlet((1, 1, 1), n - 2 * k).astype(np.float32)
    o[2 * k :] = (p[pick] * w[:, :, None]).sum(1)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= rng.uniform(0.25, 4.0, (n, 1)).astype(np.float32)
    outside = np.arange(n) >= k
    outside &= np.arange(n) < 2 * k
    d[outside] = (c - o[outside]) * rng.uniform(0.1, 1.0, (outside.sum(), 1)).astype(np.float32)  # aimed at the box, non-unit
    t = np.full(n, np.finfo(np.float32).max, np.float32)
    sel = rng.random(n)
    t[sel < 0.2] = rng.uniform(0.5, 4.0, (sel < 0.2).sum())  # finite: may or may not reach the first hit
    t[(sel >= 0.2) & (sel < 0.3)] = 1e-6  # shorter than any hit
    short = (sel >= 0.2) & (sel < 0.3) & (np.arange(n) < 2 * k)  # (an origin ON a surface may still hit at t = 0: not counted)
    return np.concatenate([o, d, t[:, None]], axis=1).astype(np.float32), short


def random_rays(rng, n, scale=1.0):
    r = np.zeros((n, 7), np.float32)
    r[:, 0:3] = rng.uniform(-2, 2, (n, 3)) * scale
    d = rng.normal(size=(n, 3))
    r[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 6] = FMAX
    return r


def primitive_inputs():
    """The seeded inputs of the element-wise primitive checks, shared by the bit-parity tests (device against oracle) and the referee's
    tests (both against float64): triangle rows with on-plane, tiny and scaled cases, planes' triangles incl. degenerate ones, boxes with
    flat ones, zero direction components and origins on faces, spheres; finite ray.t mixed in."""
    out = {}
    rng = np.random.RandomState(11)
    n = 200_000
    tri = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    r = random_rays(rng, n)
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    tgt = w[:, 0:1] * tri[:, 0:3] + w[:, 1:2] * tri[:, 3:6] + w[:, 2:3] * tri[:, 6:9]
    d = tgt - r[:, 0:3]
    r[: n // 2, 3:6] = (d / np.linalg.norm(d, axis=1, keepdims=True))[: n // 2]
    r[::7, 6] = rng.uniform(0, 3, len(r[::7]))
    tri[:1000, [2, 5, 8]] = 0.5
    r[:1000, 2] = 0.5
    tri[1000:2000] *= np.float32(1e-18)
    r[1000:2000, 0:3] *= np.float32(1e-18)
    r[2000:3000, 3:6] *= np.float32(1e-20)
    r[3000:4000, 3:6] *= np.float32(1e15)
    out["triangle"] = (tri, r)

    rng = np.random.RandomState(12)
    n = 100_000
    tri9 = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    tri9[:500] *= np.float32(1e-15)
    tri9[500:600, 3:6] = tri9[500:600, 0:3]
    out["tri9"] = tri9
    r = random_rays(rng, n)
    r[::5, 6] = rng.uniform(0, 3, len(r[::5]))
    r[:2000, 3:6] = 0.0
    out["plane_rays"] = r
    out["pin_points"] = rng.uniform(-1, 1, (n, 3)).astype(np.float32)

    rng3 = np.random.RandomState(13)
    n = 200_000
    lo = rng3.uniform(-1, 0.5, (n, 3)).astype(np.float32)
    hi = (lo + rng3.uniform(0, 1, (n, 3))).astype(np.float32)
    hi[:5000, 0] = lo[:5000, 0]
    box = np.concatenate([lo, hi], 1)
    r = random_rays(rng3, n)
    r[0:20000:2, 3] = 0.0
    r[1:20000:2, 4] = -0.0
    r[20000:30000, 3:5] = 0.0
    r[30000:40000, 0] = lo[30000:40000, 0]
    r[40000:50000, 0:3] = ((lo[40000:50000].astype(np.float64) + hi[40000:50000]) / 2).astype(np.float32)
    r[50000:60000, 1] = hi[50000:60000, 1]
    r[50000:60000, 4] = 0.0
    r[::3, 6] = rng3.uniform(0, 3, len(r[::3]))
    out["box"] = (box, r)

    rng4 = np.random.RandomState(14)
    n = 100_000
    sph = np.concatenate([rng4.uniform(-1, 1, (n, 3)), rng4.uniform(0.05, 1.5, (n, 1))], 1).astype(np.float32)
    r = random_rays(rng4, n)
    d = sph[:, 0:3] - r[:, 0:3]
    r[: n // 2, 3:6] = (d / np.linalg.norm(d, axis=1, keepdims=True))[: n // 2]
    r[::4, 6] = rng4.uniform(0, 3, len(r[::4]))
    out["sphere"] = (sph, r)
    return out


def plane_and_points(inp, planes):
    """The ray-plane and point-in-triangle inputs, which depend on the planes the code under test computed from inp["tri9"]: the planes
    with rows 5000-5999 moved (nearly) through their ray's origin, and v0 v1 v2 n p rows."""
    r = inp["plane_rays"]
    pl2 = np.array(planes, np.float32)
    pl2[5000:6000, 0] = (r[5000:6000, 0:3] * pl2[5000:6000, 1:4]).astype(np.float32).sum(1)
    pin = np.concatenate([inp["tri9"], np.asarray(planes, np.float32)[:, 1:4], inp["pin_points"]], 1)
    return pl2, pin

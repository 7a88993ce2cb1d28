"""Scenes, rays and assertions that tests/test_referee_cpu.py (oracle against the float64 referee) and tests/test_referee_gpu.py (device
against it) share, so that the device gets exactly the checks, caps and exclusions the oracle gets.  Not a test module."""
import numpy as np

import hp_ref
import rayfam

U = hp_ref.U
FMAX = rayfam.FMAX
AMBIGUOUS_CAP = 0.02  # share of the non-degenerate families a scene may have flagged
UNSTABLE_CAP = 0.02  # share of a frame's pixels that may be unstable

SMALL = ("cube", "cornell", "monkey", "blob", "spheres", "mixed", "mirrorblob")  # ~40 K rays each
LARGE = ("dodge", "dragon")  # 16-20 K triangles: ~4 K rays each
CLEAR_FAMILIES = ("primary", "random_unit", "random_scaled", "finite_t", "graze_centroid", "inside_boxes", "arbitrary", "close_range", "at_spheres")
DEGENERATE = ("on_plane", "arbitrary_on_surface", "axis_parallel", "extreme", "f4_cube", "graze_vertex", "graze_edge")


def scene(pkg, scene_data, name):
    S = pkg.scenes
    if name == "mixed":  # meshes and spheres together: a sphere in front of, inside and behind the monkey
        sd = scene_data("monkey")
        sph = np.float32([[0.45, 0.3, -0.9, 0.3, -1], [0.0, 0.0, 0.0, 0.35, -1], [-0.6, -0.2, 1.4, 0.5, -1]])
        return S.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials, spheres=sph, point_lights=sd.point_lights, name=name)
    if name == "mirrorblob":
        return mirror_blob(pkg)
    if name == "dragon":
        return S.make_dragon(20_000)
    return scene_data(name)


def mirror_blob(pkg):
    """A smooth-normal mesh with mirror materials (the blob), a mirror floor under it and an occluder between it and its first light: the
    scene on which interpolated normals, shadows and mirror rays all matter at once."""
    S = pkg.scenes
    b = S.make_blob(2000, seed=7)

    def quad(p0, p1, p2, p3, nrm):
        P = np.float32([p0, p1, p2, p0, p2, p3])
        return np.concatenate([P, np.broadcast_to(np.float32(nrm), P.shape)], 1)

    floor = quad((-2.5, -1.25, -2.5), (-2.5, -1.25, 2.5), (2.5, -1.25, 2.5), (2.5, -1.25, -2.5), (0, 1, 0))
    c, t1, t2 = np.float64([-0.72, 0.72, -0.72]), 0.15 * np.float64([1, 1, 0]) / np.sqrt(2.0), 0.15 * np.float64([1, -1, -2]) / np.sqrt(6.0)
    occ = quad(c - t1 - t2, c + t1 - t2, c + t1 + t2, c - t1 + t2, (-0.577, 0.577, -0.577))  # casts a patch of shadow on the blob
    V = len(b.pos_nrm)
    pn = np.concatenate([b.pos_nrm, floor, occ]).astype(np.float32)
    # make_blob winds its triangles inwards, and the reference flips the shading normal by the *geometric* one (ray_tracing.cpp:99):
    # seen from outside the blob would be lit from within, i.e. black.  Wound outwards here, so that its shading is visible.
    tri = np.concatenate([b.tri[:, [0, 2, 1]], np.uint32([[V, V + 1, V + 2], [V + 3, V + 4, V + 5], [V + 6, V + 7, V + 8], [V + 9, V + 10, V + 11]])])
    tm = np.concatenate([b.tri_mesh, np.uint32([3, 3, 4, 4])])
    # main.cpp:246 tests ks.z alone (a comma operator): the blob's middle band gets ks.x > 0.01 >= ks.z (no mirror), its lower cap
    # ks.z > 0.01 >= ks.x (a mirror, over the floor), so that "ks.x" or "any / all components" in its place changes the frame
    bm = b.materials.copy()
    bm[1, 3:6] = (0.5, 0.5, 0.004)
    bm[2, 3:6] = (0.004, 0.9, 0.9)
    mats = np.concatenate([bm, np.float32([[0.3, 0.3, 0.35, 0.4, 0.4, 0.4, 30, 1], [0.6, 0.5, 0.1, 0, 0, 0, 1, 1]])])
    return S.SceneData(pos_nrm=pn, tri=tri.astype(np.uint32), tri_mesh=tm.astype(np.uint32), materials=mats, point_lights=b.point_lights, name="mirrorblob")


def primary_grid(cam, W, H):
    """The primary rays of a W x H frame from the referee's own camera, rounded to float32 once."""
    o, d = hp_ref.camera_rays(cam, W, H)
    return np.concatenate([o, d, np.full((len(o), 1), FMAX)], 1).astype(np.float32)


def _close_range(sd, rng, n=800):
    """Origins 3e-4 .. 8e-4 in front of a surface point, shooting back at it: clear hits at a t that an `eps` in the place of 0 would reject."""
    p = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, :3].astype(np.float64)
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    k = tri[rng.randint(0, len(tri), n)]
    w = rng.dirichlet((4, 4, 4), n)
    A, B, C = p[k[:, 0]], p[k[:, 1]], p[k[:, 2]]
    pt = w[:, 0:1] * A + w[:, 1:2] * B + w[:, 2:3] * C
    nn = np.cross(B - A, C - A)
    nn /= np.maximum(np.linalg.norm(nn, axis=1, keepdims=True), 1e-300)
    side = np.where(rng.rand(n, 1) < 0.5, 1.0, -1.0)
    d = -side * nn + 0.3 * rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = pt + side * nn * rng.uniform(3e-4, 8e-4, (n, 1))
    return np.concatenate([o, d, np.full((n, 1), FMAX)], 1).astype(np.float32)


def _at_spheres(sd, rng, n=2500):
    sp = np.asarray(sd.spheres, np.float64).reshape(-1, 5)
    k = rng.randint(0, len(sp), n)
    aim = sp[k, :3] + sp[k, 3:4] * 1.3 * rng.uniform(-1, 1, (n, 3))
    o = sp[k, :3] + sp[k, 3:4] * rng.uniform(-4, 4, (n, 3))
    o[::5] = sp[k[::5], :3] + sp[k[::5], 3:4] * rng.uniform(-0.5, 0.5, (len(o[::5]), 3))  # starts inside
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[1::4] *= rng.uniform(0.2, 5.0, (len(d[1::4]), 1))
    t = np.full(n, FMAX)
    t[2::6] = rng.uniform(0.2, 12.0, len(t[2::6]))
    return np.concatenate([o, d, t[:, None]], 1).astype(np.float32)


def ray_families(pkg, orc, sd, name):
    """name -> (n, 7) float32 rays: the rayfam families (its own seed), rayfam.arbitrary_rays, and two families of this module."""
    large = name in LARGE
    W = 48 if large else 160
    cam = pkg.scenes.default_camera(W, W)
    prim = primary_grid(cam, W, W)
    _, boxes = orc.OracleScene(sd).nodes()
    fam = rayfam.families(sd, boxes, prim, rng=np.random.RandomState(rayfam.SEED & 0x7FFFFFFF), n_random=150 if large else 1500)
    rng = np.random.RandomState(20241)
    if sd.ntris:
        arb = rayfam.arbitrary_rays(sd, 400 if large else 4000, seed=5)[0]
        k = 2 * (len(arb) // 3)  # the last third starts ON the surfaces: degenerate by construction, like on_plane
        fam["arbitrary"], fam["arbitrary_on_surface"] = arb[:k], arb[k:]
        fam["close_range"] = _close_range(sd, rng, 80 if large else 800)
    if len(sd.spheres):
        fam["at_spheres"] = _at_spheres(sd, rng)
    if large:  # a tenth of every family, as the primary grid and the random families already are: the mix stays that of the small scenes
        for k in DEGENERATE + ("graze_centroid", "inside_boxes"):
            if k in fam and k != "f4_cube":
                fam[k] = fam[k][::10]
    return fam


def concat(fam):
    names = sorted(fam)
    spans, at = {}, 0
    for k in names:
        spans[k] = slice(at, at + len(fam[k]))
        at += len(fam[k])
    return np.concatenate([fam[k] for k in names]).astype(np.float32), spans


def in_families(spans, n, which):
    m = np.zeros(n, bool)
    for k in which:
        if k in spans:
            m[spans[k]] = True
    return m


def class_report(ref, mask):
    return ", ".join(f"{k}: {int((ref['flags'][k] & mask).sum())}" for k in hp_ref.CLASSES)


def check_caps(name, ref, spans):
    """The ambiguous share of the non-degenerate families stays under the cap; the assertion message carries the share per class."""
    n = len(ref["hit"])
    m = in_families(spans, n, CLEAR_FAMILIES)
    share = float((ref["amb"] & m).sum()) / max(int(m.sum()), 1)
    print(f"[referee] {name}: {int(m.sum())} rays in non-degenerate families, ambiguous share {share:.4%} ({class_report(ref, m)}), hits {ref['hit'][m].mean():.3f}")
    assert share <= AMBIGUOUS_CAP, f"{name}: {share:.3%} of the non-degenerate rays are ambiguous (cap {AMBIGUOUS_CAP:.0%}); per class {class_report(ref, m)}"
    return m & ~ref["amb"]


def as_got(hit, t, prim, material, normal):
    prim = np.asarray(prim).astype(np.int64)
    return dict(hit=np.asarray(hit) != 0, t=np.asarray(t, np.float32).astype(np.float64), prim=np.where(prim == 0xFFFFFFFF, -1, prim),
                material=np.asarray(material).astype(np.int64), normal=None if normal is None else np.asarray(normal, np.float64))


def check_hits(label, ref, got, clear, exact_prim=True):
    """On the clear rays: flag equal, primitive equal, t and normal within their derived bounds, material equal.  Returns the largest
    t error in units of 2^-24 * cond and the largest normal error over its bound."""
    bad = clear & (got["hit"] != ref["hit"])
    assert not bad.any(), f"{label}: verdict differs on {int(bad.sum())} clear rays, first {np.nonzero(bad)[0][:5]} (true hits missed: {int((bad & ref['hit']).sum())})"
    both = clear & ref["hit"]
    if exact_prim:
        bad = both & (got["prim"] != ref["prim"])
        assert not bad.any(), f"{label}: primitive differs on {int(bad.sum())} clear rays, first {np.nonzero(bad)[0][:5]}"
    K = np.where(ref["sphere"], hp_ref.K_S, hp_ref.K_T)
    with np.errstate(all="ignore"):
        rel = np.abs(got["t"] - ref["t"]) / ref["t"]
        unit = rel / (U * ref["cond"])
    bad = both & ~(unit <= K)
    worst = float(unit[both].max(initial=0.0))
    assert not bad.any(), (f"{label}: t outside K * 2^-24 * cond on {int(bad.sum())} clear rays, worst {worst:.3g} units (K = {K[bad][0]}), "
                           f"first {np.nonzero(bad)[0][:5]}, rel {rel[bad][:3]}")
    bad = both & (got["material"] != ref["material"])
    assert not bad.any(), f"{label}: material differs on {int(bad.sum())} clear rays, first {np.nonzero(bad)[0][:5]}"
    nworst = 0.0
    if got["normal"] is not None:
        ang = hp_ref.angle(got["normal"], ref["normal"])
        over = np.where(both, ang / ref["nbound"], 0.0)
        nworst = float(np.nanmax(over, initial=0.0))
        bad = both & ~(ang <= ref["nbound"])
        assert not bad.any(), (f"{label}: normal outside its bound on {int(bad.sum())} clear rays, worst {nworst:.3g} x bound, first {np.nonzero(bad)[0][:5]}, "
                               f"angle {ang[bad][:3]} bound {ref['nbound'][bad][:3]}")
        ln = np.sqrt((got["normal"] ** 2).sum(-1))
        assert np.all(np.abs(ln[both] - 1) < 16 * U), f"{label}: a hit normal is not unit length"
    print(f"[referee] {label}: {int(both.sum())} clear hits, worst t error {worst:.3f} x 2^-24 cond (allowed {hp_ref.K_T:g}), worst normal {nworst:.3f} x bound")
    return worst, nworst


def check_no_false_miss(label, ref, got, spans):
    """(Implied by check_hits' first assertion; kept for its message, not a second check.)  Every miss of a true hit is an ambiguous ray (the reference tree's known false misses come from flat boxes and grazing rays).
    The three recorded cube rays (rayfam.F4_*) are the named exception: the reference's own tree misses them, and the referee agrees
    with the reference's brute force on them instead (check_f4)."""
    m = in_families(spans, len(ref["hit"]), CLEAR_FAMILIES)
    bad = m & ref["hit"] & ~got["hit"] & ~ref["amb"]
    assert not bad.any(), f"{label}: {int(bad.sum())} clear rays with a true hit are reported as misses, first {np.nonzero(bad)[0][:5]}"


def check_degenerate_flagged(name, R, rays, ref, spans):
    """on_plane: every ray is class e.  graze_vertex / graze_edge: every ray whose grazed feature is not hidden behind a nearer hit is
    flagged, unless float32's rounding of the direction carried it further than the band from the feature (reported, with the distance)."""
    for fam in ("on_plane", "arbitrary_on_surface"):
        if fam in spans:
            e = ref["flags"]["e"][spans[fam]]
            assert e.all(), f"{name}: {int((~e).sum())} {fam} rays are not class e"
    P = np.asarray(R.A), np.asarray(R.B)
    for fam, pts in (("graze_vertex", P[0]), ("graze_edge", 0.5 * (P[0] + P[1]))):
        if fam not in spans:
            continue
        r = rays[spans[fam]].astype(np.float64)
        o, d = r[:, :3], r[:, 3:6]
        rel = pts[None] - o[:, None]
        tp = (rel * d[:, None]).sum(-1) / (d * d).sum(-1)[:, None]
        off = np.linalg.norm(rel - tp[..., None] * d[:, None], axis=-1)
        k = off.argmin(1)
        tP = tp[np.arange(len(k)), k]
        h, t, amb = ref["hit"][spans[fam]], ref["t"][spans[fam]], ref["amb"][spans[fam]]
        visible = ~(h & (t < tP * (1 - 1e-4)))
        miss = visible & ~amb
        # The independent quantity: the ray passes the grazed point at perpendicular distance `off`.  In the plane of triangle k that is at
        # most off / cos away from the point, and a barycentric weight changes by at most 1 / h_min per unit length (h_min: the
        # triangle's smallest height), so off / (cos * h_min) < BAND puts the plane hit inside the edge band: such a ray must be flagged.
        rows = np.arange(len(k))
        cos = np.abs((d * R.gn[k]).sum(-1)) / np.linalg.norm(d, axis=1)
        reach = off[rows, k] / np.maximum(cos * R.area2[k] / R.longest[k], 1e-300)
        if miss.any():
            print(f"[referee] {name}/{fam}: {int(miss.sum())} of {int(visible.sum())} visible rays are not flagged: float32's rounding of the direction "
                  f"carried them {reach[miss].min():.3g} .. {reach[miss].max():.3g} (barycentric reach, band {hp_ref.BAND:g}) from the feature; "
                  f"perpendicular distance up to {off[rows, k][miss].max():.3g}")
        assert (reach[miss] >= hp_ref.BAND).all(), f"{name}/{fam}: a ray within the band of a visible grazed feature is not flagged"
        print(f"[referee] {name}/{fam}: {int(visible.sum())} of {len(k)} features visible, {int((visible & amb).sum())} flagged")


def check_f4(name, R, rays, ref, spans):
    """The three recorded cube rays (rayfam.F4_*): each runs along the diagonal of a cube face, i.e. exactly through the edge two
    triangles share, which is why the reference's tree and its brute force could disagree on them.  The referee must class them a
    (edge band), and its t on that edge must be what the unmodified reference's brute force printed, to all nine digits given."""
    if name != "cube" or "f4_cube" not in spans:
        return
    sl = spans["f4_cube"]
    assert ref["flags"]["a"][sl].all(), "the recorded cube rays are not classed as edge hits"
    r = rays[sl].astype(np.float64)
    t, u, v, det, _ = R._triangles(r[:, :3], r[:, 3:6])
    mb = np.minimum(np.minimum(u, v), 1 - u - v)
    k = np.where(t > 0, mb, -np.inf).argmax(1)
    got = t[np.arange(3), k]
    want = np.array([float(x) for x in rayfam.F4_BRUTE_T])
    assert np.all(np.abs(mb[np.arange(3), k]) < hp_ref.BAND)
    assert np.all(np.abs(got - want) <= 2 * U * want), f"the referee's t {got} on the recorded cube rays is not the reference brute force's {want}"
    print(f"[referee] cube/f4: referee t {got} against the reference's printed {want}: within {np.max(np.abs(got - want) / want) / U:.2f} u")


# ---------------------------------------------------------------------------------------------------------------------------------
# shading
# ---------------------------------------------------------------------------------------------------------------------------------
THREE_LIGHTS = np.float32([[0.0, 0.58, 0.0, 1, 1, 1], [0.4, -0.3, -0.5, 0.2, 0.7, 0.3], [1.6, 0.2, 0.1, 0.9, 0.2, 0.2]])  # the last: behind Cornell's wall
SHADE_W = 96
# frame name -> (scene, lights (None: the scene's own), depth); the rays are the default camera's (spheres: a camera facing them)
FRAMES = {
    "cornell_d1": ("cornell", None, 1), "cornell_d2": ("cornell", None, 2), "cornell_d4": ("cornell", None, 4),
    "cornell_3l_d1": ("cornell", THREE_LIGHTS, 1), "cornell_3l_d2": ("cornell", THREE_LIGHTS, 2), "cornell_3l_d4": ("cornell", THREE_LIGHTS, 4),
    "monkey_d2": ("monkey", None, 2), "spheres_d2": ("spheres", None, 2), "mixed_d2": ("mixed", None, 2),
    "mirrorblob_d3": ("mirrorblob", None, 3), "mirrorblob_scaled_d3": ("mirrorblob", None, 3),
}
# frames whose rays are the camera's with the direction of even pixels halved and of odd pixels tripled: the mirror ray's limit is
# |direction| (main.cpp:254), which unit-length camera rays cannot tell from the constant 1.  Ray lists only (no camera gives them).
SCALED = ("mirrorblob_scaled_d3",)
# Largest |RGB error| of the oracle (float32, libm powf) against hp_ref.shade over the stable pixels of each scene's frames above,
# measured on the CPU (tests/test_referee_cpu.py prints it; never measured on the device).  The CPU test allows the oracle 1.5 x this,
# the GPU test allows the device 4 x: device powf differs from libm's by a few ulp, amplified by the shininess; a wrong term shows up
# at 1e-2 and above.  Kept per scene: one global figure would be set by the glossiest material and blunt the rest.
RGB_MEASURED = {
    "cornell": 7.6e-7,  # cornell_3l_d1 (2.2e-7 under its own single light)
    "monkey": 4.6e-5,  # monkey_d2: shininess 225, two lights
    "mixed": 7.4e-5,  # mixed_d2: the monkey's material on spheres
    "mirrorblob": 1.9e-6,  # mirrorblob_d3 (1.82e-6; mirrorblob_scaled_d3 the same)
    "spheres": 0.0,  # spheres_d2: a sphere-only hit has the default material, kd = ks = 0: every term is an exact zero
}
RGB_DEVICE_FACTOR = 4.0


def frame_lights(sd, lights):
    return np.asarray(sd.point_lights if lights is None else lights, np.float32).reshape(-1, 6)


def check_rgb(label, want, unstable, got, bound):
    share = float(unstable.mean())
    assert share <= UNSTABLE_CAP, f"{label}: {share:.3%} of the pixels are unstable (cap {UNSTABLE_CAP:.0%})"
    err = np.abs(np.asarray(got, np.float64).reshape(-1, 3) - want).max(1)
    stable = ~unstable
    worst = float(err[stable].max(initial=0.0))
    at = int(np.nonzero(stable)[0][err[stable].argmax()]) if stable.any() else -1
    print(f"[referee] {label}: unstable {share:.3%}, largest |dRGB| on stable pixels {worst:.3e} at pixel {at} (allowed {bound:.3e}), over all pixels {err.max():.3e}, "
          f"mean rgb {want.mean():.4f}")
    assert worst <= bound, f"{label}: |dRGB| {worst:.3e} at pixel {at} (want {want[at]}, got {np.asarray(got).reshape(-1, 3)[at]}) exceeds {bound:.3e}"
    return worst


class Frames:
    """The referee's frames, computed once per test module (a module-scoped fixture holds one of these)."""

    def __init__(self):
        self._done = {}

    def frame(self, pkg, orc, scene_data, frame):
        """(sd, cam, rays, lights, depth, rgb, unstable, why) of a frame of FRAMES; cam is None for the frames of SCALED."""
        if frame not in self._done:
            name, lights, depth = FRAMES[frame]
            sd = scene(pkg, scene_data, name)
            W = SHADE_W
            cam = pkg.scenes.default_camera(W, W)
            if name == "spheres":  # the preset's spheres stand at z = 4 .. 10: look at them
                cam = np.float32([0, 0, 6, 0, 0, 0, 9.0, cam[7], 1.0])
            rays = orc.generate_rays(cam, W, W)  # held against hp_ref.camera_rays by the camera tests
            if frame in SCALED:
                rays = rays.copy()
                rays[0::2, 3:6] *= np.float32(0.5)
                rays[1::2, 3:6] *= np.float32(3.0)
                cam = None
            self.extra(frame, pkg, scene_data, name, rays, cam, lights, depth)
        return self._done[frame]

    def extra(self, key, pkg, scene_data, name, rays, cam, lights, depth):
        """A frame of other rays of one of the scenes (another camera), kept like the rest."""
        if key not in self._done:
            sd = scene(pkg, scene_data, name)
            L = frame_lights(sd, lights)
            rgb, unstable, why = hp_ref.Referee(sd).shade(rays, L, depth)
            self._done[key] = (sd, cam, rays, L, depth, rgb, unstable, why)
        return self._done[key]

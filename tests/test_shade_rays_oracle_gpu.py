"""cgrt_shade_rays (Scene.shade_rays) against the CPU oracle's own ray-list entry (OracleScene.shade_rays): RGB within 1e-5, NaN at
the same positions, equal ray counts of every kind.  Until these tests, ray lists were only checked against the C++ mirror, whose
intersections run on the library's own device boundary.

* Scenes: cube, monkey, Cornell, Cornell with spheres in front of its walls (a sphere hit after a wall keeps the wall's material,
  bvh.cpp:878-879, and shades with it), and that box with every material a mirror (recursion to depth 16).
* Rays: every family of tests/rayfam.py (axis-parallel, origins on boxes and planes, grazing, finite t, extreme magnitudes, the F4
  cube rays), rayfam.arbitrary_rays (non-unit directions: the mirror ray's t = |r.d|, main.cpp:254), and degenerate rays.
* Depths 0, 1, 2, 4, 16; point lights, spherical lights, both, and 8 point lights (some outside the scene, one on a surface).
* Every forced kernel shape and both walks give the auto shape's colours bit for bit."""
import numpy as np
import pytest
import rayfam
from conftest import same_bits

pytestmark = pytest.mark.gpu

THREADS = 16
DEPTHS = (0, 1, 2, 4, 16)
SHAPES = (-1, 0, 1, 2, 3)  # cgrt_set_kernel_shape: auto, LANE64, QUAD16, LANE16, QUAD4 (as tests/test_shade_rays_gpu.py)
MAX_RAYS = 6000  # per scene: a seeded subset of the families, keeping the F4 and degenerate rays
SPHERES = np.float32([[0.1, -0.2, 0.0, 0.25, -1], [-0.3, 0.2, 0.1, 0.2, -1]])


def _scene(pkg, scene_data, name):
    if name in ("cube", "monkey", "cornell"):
        return scene_data(name)
    sd = scene_data("cornell")
    mats = sd.materials.copy()
    if name == "cornell_mirrors":
        mats[:, 3:6] = np.float32(0.6)  # every surface reflects: paths that only end at max_level
        mats[:, 6] = np.float32(20.0)
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=mats, spheres=SPHERES,
                                point_lights=sd.point_lights)


def _degenerate():
    """Zero direction, denormal components, t = 0 and t = inf, from inside and outside the unit-sized scenes."""
    dn = np.float32(1e-40)
    rows = []
    for o in ((0.0, 0.1, 0.0), (0.3, 0.2, -2.5), (1.1, 1.3, -2.6)):
        for d, t in (((0, 0, 0), rayfam.FMAX), ((dn, dn, dn), rayfam.FMAX), ((0, 0, dn), rayfam.FMAX), ((dn, 0, 1), rayfam.FMAX),
                     ((0.1, -0.2, 1.0), 0.0), ((0.1, -0.2, 1.0), np.inf), ((0, -dn, 1), 0.0), ((-0.0, -0.0, 1.0), rayfam.FMAX)):
            rows.append([*o, *d, t])
    return np.asarray(rows, np.float32)


def _rays(pkg, orc, sd, o):
    W = H = 24
    primary = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    _, boxes = o.nodes()
    fam = rayfam.families(sd, boxes, primary)
    keep = [fam.pop("f4_cube"), _degenerate()]
    rest = rayfam.concat(fam)
    rng = np.random.default_rng(0xC0FFEE)
    arb, _ = rayfam.arbitrary_rays(sd, 600, 7) if sd.ntris else (np.zeros((0, 7), np.float32), None)
    rest = np.concatenate([rest[rng.choice(len(rest), min(len(rest), MAX_RAYS - 600), replace=False)], arb])
    return np.ascontiguousarray(np.concatenate(keep + [rest]), np.float32)


def _lights(pkg, sd, kind):
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3]
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, (hi - lo) / 2
    top = c + np.float32([0.0, 0.8, 0.0]) * ext
    point = np.concatenate([np.asarray(sd.point_lights, np.float32).reshape(-1, 6), [[*top, 0.6, 0.7, 0.8]]]).astype(np.float32)
    spherical = np.float32([[*top, 0.08, 1.0, 0.9, 0.8], [*(c + np.float32([-0.5, 0.3, -1.5]) * ext), 0.3, 0.5, 0.5, 0.7]])
    soft = dict(spherical=spherical, units=pkg.unit_vector_table(1000, 5), samples=6, seed=123)
    if kind == "point":
        return point, {}
    if kind == "spherical":
        return np.zeros((0, 6), np.float32), soft
    if kind == "both":
        return point, soft
    assert kind == "eight"
    tri = np.asarray(sd.tri, np.int64)[0]
    on_surface = p[tri].astype(np.float64).mean(0).astype(np.float32)  # a triangle's centroid: a light ON the mesh
    pos = np.float32([c + 0.5 * ext, c - 0.5 * ext, c + [0, 0, 3.0], c + [9.0, 0, 0], c - [0, 40.0, 0], c + [0.2, 0.1, -0.3] * ext,
                      [-1e3, 2e3, 5e2], on_surface])
    col = np.random.default_rng(8).uniform(0.1, 0.5, (8, 3)).astype(np.float32)
    return np.concatenate([pos, col], 1).astype(np.float32), {}


def _assert_matches(got, gst, want, wc, what):
    nan = np.isnan(got) | np.isnan(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions differ", int(nan.sum()))
    eq = same_bits(got, want)
    with np.errstate(invalid="ignore"):  # (inf - inf where the bits are equal: masked by eq)
        err = np.where(eq, 0.0, np.abs(got.astype(np.float64) - want))
    assert not np.isnan(err).any() and float(err.max(initial=0.0)) <= 1e-5, (what, float(np.nanmax(err, initial=0.0)))
    for k, v in wc.items():
        assert gst[k] == v, (what, k, gst[k], v)


@pytest.fixture(scope="module")
def cases(pkg, orc, scene_data):
    made = {}
    for name in ("cube", "monkey", "cornell", "cornell_spheres", "cornell_mirrors"):
        sd = _scene(pkg, scene_data, name)
        o = orc.OracleScene(sd)
        made[name] = (sd, o, pkg.Scene(sd, device=0), _rays(pkg, orc, sd, o))
    yield made
    for _, o, sc, _ in made.values():
        sc.close()
        o.close()


@pytest.mark.parametrize("name", ["cube", "monkey", "cornell", "cornell_spheres", "cornell_mirrors"])
@pytest.mark.parametrize("kind", ["point", "spherical", "both", "eight"])
def test_shade_rays_match_the_oracle(pkg, cases, name, kind):
    sd, o, sc, rays = cases[name]
    lights, soft = _lights(pkg, sd, kind)
    depths = DEPTHS if name != "cornell_mirrors" else (2, 16)
    for depth in depths:
        want, wc = o.shade_rays(rays, lights, max_level=depth, threads=THREADS, **soft)
        got, gst = sc.shade_rays(rays, lights=lights, max_level=depth, **soft)
        _assert_matches(got, gst, want, wc, (name, kind, depth))
        if depth >= 1:
            assert wc["primary_rays"] == len(rays)
            assert (wc["shadow_rays"] > 0) == (kind != "spherical") and (wc["soft_shadow_rays"] > 0) == bool(soft)
        if depth >= 2 and name != "cube":
            assert wc["reflection_rays"] > 0
        if name == "cornell_mirrors" and depth == 16:
            assert wc["reflection_rays"] > 3 * len(rays), "mirror paths must reach deep levels"


def test_stale_sphere_material_shades_visibly(pkg, orc, cases):
    """Sphere hits after a wall hit keep the wall's material: the oracle shades them, and so must the device (not black)."""
    sd, o, sc, _ = cases["cornell_spheres"]
    W = H = 64
    rays = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    hit = o.intersect(rays)
    stale = (hit["hit"] == 1) & (hit["prim"] >= sd.ntris) & (hit["material"] >= 0)
    assert stale.sum() > 50
    lights, soft = _lights(pkg, sd, "both")
    want, wc = o.shade_rays(rays, lights, max_level=2, threads=THREADS, **soft)
    got, gst = sc.shade_rays(rays, lights=lights, max_level=2, **soft)
    _assert_matches(got, gst, want, wc, "stale")
    assert (want[stale].max(1) > 0).mean() > 0.5


def test_kernel_shapes_and_walks_agree(pkg, cases):
    sd, o, sc, rays = cases["cornell_spheres"]
    lights, soft = _lights(pkg, sd, "both")
    auto, ast = sc.shade_rays(rays, lights=lights, max_level=4, **soft)
    try:
        for certified in (True, False):
            sc.set_walk(certified)
            for mode in SHAPES:
                pkg.set_kernel_shape(mode)
                got, gst = sc.shade_rays(rays, lights=lights, max_level=4, **soft)
                assert got.tobytes() == auto.tobytes(), (certified, mode)
                assert all(gst[k] == ast[k] for k in ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays"))
            pkg.set_kernel_shape(-1)
    finally:
        pkg.set_kernel_shape(-1)
        sc.set_walk(True)

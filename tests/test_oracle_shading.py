"""The oracle's shading entries among themselves (CPU only): oracle_shade_rays (getFinalColor of a caller's ray list) and the ray
counts by kind of every shading entry.

* The camera's rays, shaded as a list, equal the oracle's own frame bit for bit, with equal counts by kind: list hashing (sample smp
  of ray i with pixel i) is frame hashing (pixel y * W + x) for the camera's row-major rays.
* Edges: max_level 0, t shorter than the first hit, a spherical light of radius 0, a one-entry unit table, one sample.
* The counts by kind add up to the single total the frame entries have always returned."""
import numpy as np
import pytest
from conftest import same_bits

THREADS = 8  # the oracle never needs more for these frames
NONE = np.zeros((0, 6), np.float32)


def _soft(pkg, samples=16, seed=11, nunits=4096):
    return dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(nunits, 3), samples=samples, seed=seed)


def _with_spheres(pkg, sd):
    """The Cornell box with two spheres in front of its walls (as tests/test_parity_gpu.py test_mixed_meshes_and_spheres)."""
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials, point_lights=sd.point_lights,
                                spheres=np.float32([[0.1, -0.2, 0.0, 0.25, -1], [-0.3, 0.2, 0.1, 0.2, -1]]))


@pytest.fixture(scope="module")
def oscenes(pkg, orc, scene_data):
    sds = {n: scene_data(n) for n in ("cube", "monkey", "cornell")}
    sds["cornell_spheres"] = _with_spheres(pkg, sds["cornell"])
    return {n: (sd, orc.OracleScene(sd)) for n, sd in sds.items()}


@pytest.mark.parametrize("name", ["cube", "monkey", "cornell", "cornell_spheres"])
@pytest.mark.parametrize("W,H", [(1, 1), (13, 7), (40, 24)])
def test_camera_rays_as_a_list_equal_the_frame(pkg, orc, oscenes, name, W, H):
    sd, o = oscenes[name]
    cam = pkg.scenes.default_camera(W, H)
    rays = orc.generate_rays(cam, W, H)
    soft = _soft(pkg, samples=8)
    for depth in (0, 1, 2, 4):
        want, wc = o.render(cam, W, H, sd.point_lights, max_level=depth, threads=THREADS, by_kind=True)
        got, gc = o.shade_rays(rays, sd.point_lights, max_level=depth, threads=THREADS)
        assert same_bits(got, want).all(), (name, W, H, depth)
        assert gc == wc, (name, W, H, depth, gc, wc)
        assert gc["primary_rays"] == (W * H if depth >= 1 else 0) and gc["soft_shadow_rays"] == 0
        want, wc = o.render_soft(cam, W, H, sd.point_lights, max_level=depth, threads=THREADS, by_kind=True, **soft)
        got, gc = o.shade_rays(rays, sd.point_lights, max_level=depth, threads=THREADS, **soft)
        assert same_bits(got, want).all(), ("soft", name, W, H, depth)
        assert gc == wc, ("soft", name, W, H, depth, gc, wc)


def test_list_samples_hash_with_the_ray_index(pkg, orc, oscenes):
    """A penumbra ray moved to another index draws other samples: the list's hash key is the index, not the ray."""
    sd, o = oscenes["cornell"]
    W, H = 40, 24
    rays = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    soft = _soft(pkg, samples=8)
    base, _ = o.shade_rays(rays, NONE, max_level=1, threads=THREADS, **soft)
    perm = np.random.default_rng(2).permutation(len(rays))
    moved, _ = o.shade_rays(rays[perm], NONE, max_level=1, threads=THREADS, **soft)
    assert not np.array_equal(moved, base[perm])
    shifted, _ = o.shade_rays(np.concatenate([rays[:1], rays]), NONE, max_level=1, threads=THREADS, **soft)
    assert not np.array_equal(shifted[1:], base), "p = i + 1 must draw other samples"


def test_max_level_zero_is_black_and_casts_nothing(pkg, orc, oscenes):
    sd, o = oscenes["cornell_spheres"]
    rays = orc.generate_rays(pkg.scenes.default_camera(16, 16), 16, 16)
    rgb, c = o.shade_rays(rays, sd.point_lights, max_level=0, threads=THREADS, **_soft(pkg))
    assert not rgb.any() and all(v == 0 for v in c.values())
    rgb, c = o.shade_rays(np.zeros((0, 7), np.float32), sd.point_lights, max_level=4, threads=THREADS)
    assert rgb.shape == (0, 3) and all(v == 0 for v in c.values())


def test_t_shorter_than_the_first_hit_is_black(pkg, orc, oscenes):
    sd, o = oscenes["cornell"]
    rays = orc.generate_rays(pkg.scenes.default_camera(24, 24), 24, 24)
    hit = o.intersect(rays)
    m = hit["hit"] == 1
    assert m.sum() > 100
    short = rays[m].copy()
    short[:, 6] = hit["t"][m] * np.float32(0.5)
    rgb, c = o.shade_rays(short, sd.point_lights, max_level=4, threads=THREADS, **_soft(pkg))
    assert not rgb.any()
    assert c["primary_rays"] == len(short) and c["shadow_rays"] == 0 and c["reflection_rays"] == 0 and c["soft_shadow_rays"] == 0
    # the same rays with t just beyond the hit are shaded
    far = rays[m].copy()
    far[:, 6] = hit["t"][m] * np.float32(1.01)
    rgb, _ = o.shade_rays(far, sd.point_lights, max_level=4, threads=THREADS)
    assert (rgb.max(1) > 0).sum() > len(far) // 2


def test_zero_radius_is_a_point_light(pkg, orc, oscenes):
    """As tests/test_soft_shadows.py test_oracle_soft_radius_zero_is_a_point_light, for ray lists (mirrors at depth included)."""
    sd, o = oscenes["cornell"]
    rays = orc.generate_rays(pkg.scenes.default_camera(32, 24), 32, 24)
    sl = np.asarray([[0, 0.58, 0, 0.0, 1, 1, 1]], np.float32)
    for depth in (1, 3):
        soft, cs = o.shade_rays(rays, NONE, sl, pkg.unit_vector_table(64, 1), samples=3, max_level=depth, threads=THREADS)
        hard, ch = o.shade_rays(rays, np.asarray([[0, 0.58, 0, 1, 1, 1]], np.float32), max_level=depth, threads=THREADS)
        assert np.abs(soft - hard).max() <= 1e-6
        assert cs["soft_shadow_rays"] == 3 * ch["shadow_rays"] and cs["shadow_rays"] == 0
        assert cs["primary_rays"] == ch["primary_rays"] and cs["reflection_rays"] == ch["reflection_rays"]


def test_one_unit_and_one_sample(pkg, orc, oscenes):
    """nunits = 1: every sample draws the same vector, so any sample count gives the one-sample colour exactly (counter k/k)."""
    sd, o = oscenes["cornell_spheres"]
    rays = orc.generate_rays(pkg.scenes.default_camera(32, 24), 32, 24)
    one = dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(1, 4))
    a, ca = o.shade_rays(rays, sd.point_lights, samples=1, seed=5, max_level=2, threads=THREADS, **one)
    b, cb = o.shade_rays(rays, sd.point_lights, samples=7, seed=9, max_level=2, threads=THREADS, **one)
    assert same_bits(a, b).all()
    assert cb["soft_shadow_rays"] == 7 * ca["soft_shadow_rays"] > 0
    assert a.any()
    with pytest.raises(ValueError):
        o.shade_rays(rays, sd.point_lights, samples=0, max_level=2, **one)


@pytest.mark.parametrize("name", ["cube", "monkey", "cornell", "cornell_spheres"])
def test_counts_by_kind_add_up_to_the_total(pkg, orc, oscenes, name):
    sd, o = oscenes[name]
    W, H = 32, 24
    cam = pkg.scenes.default_camera(W, H)
    soft = _soft(pkg, samples=4)
    for depth in (1, 2, 4):
        _, n = o.render(cam, W, H, sd.point_lights, max_level=depth, threads=THREADS)
        _, c = o.render(cam, W, H, sd.point_lights, max_level=depth, threads=THREADS, by_kind=True)
        assert sum(c.values()) == n and c["soft_shadow_rays"] == 0, (name, depth, c, n)
        _, n = o.render_soft(cam, W, H, sd.point_lights, max_level=depth, threads=THREADS, **soft)
        _, c = o.render_soft(cam, W, H, sd.point_lights, max_level=depth, threads=THREADS, by_kind=True, **soft)
        assert sum(c.values()) == n, (name, depth, c, n)
        assert c["primary_rays"] == W * H
        if c["primary_rays"] and c["shadow_rays"]:
            assert c["shadow_rays"] % len(sd.point_lights) == 0
            assert c["soft_shadow_rays"] == c["shadow_rays"] // len(sd.point_lights) * 4  # one sphere, 4 samples per hit


def test_stale_sphere_material_is_shaded(pkg, orc, oscenes):
    """A sphere in front of a wall the ray already hit keeps the wall's material (bvh.cpp:878-879); a sphere hit alone shades with
    the default material (black diffuse and specular).  Both kinds occur in the mixed scene's frame."""
    sd, o = oscenes["cornell_spheres"]
    W, H = 40, 40
    rays = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    hit = o.intersect(rays)
    on_sphere = (hit["hit"] == 1) & (hit["prim"] >= sd.ntris)
    stale = on_sphere & (hit["material"] >= 0)
    assert stale.sum() > 20
    rgb, _ = o.shade_rays(rays, sd.point_lights, max_level=1, threads=THREADS)
    assert (rgb[stale].max(1) > 0).sum() > stale.sum() // 2

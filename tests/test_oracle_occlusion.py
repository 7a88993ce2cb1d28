"""The CPU side of the occlusion checks (tests/test_occlusion_gpu.py): the oracle's soft-shadow counts (OracleScene.soft_lit, the loop
Shader::shading runs for spherical lights) against its own closest hit on the sample rays, rebuilt here in float32 from
main.cpp:173-199 and the unit-table hash of include/cgrt.h; the -O0 and -O2 oracle builds agree; and the ray families of
tools/occlfam.py are what they claim to be (the boundary family straddles the verdict's threshold)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import occlfam  # noqa: E402


def _fmix32(h):
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def _unit_index(seed, pixel, level, light, smp, nunits):
    h = _fmix32(np.uint64(seed) ^ np.uint64(0x9E3779B9))
    h = _fmix32(h ^ np.asarray(pixel, np.uint64))
    h = _fmix32(h ^ ((np.uint64(level) * np.uint64(0x01000193) + np.uint64(light)) & np.uint64(0xFFFFFFFF)))
    h = _fmix32(h ^ np.asarray(smp, np.uint64))
    return (h % np.uint64(nunits)).astype(np.int64)


def _items(pkg, orc, sd, o, n=300, seed=3):
    rng = np.random.default_rng(seed)
    rays = occlfam.aimed_rays(sd, n, rng)
    rays[::10, 3:6] *= np.float32(-1.0)  # away from the scene: items that missed
    ref = o.intersect(rays)
    r = rays.copy()
    r[:, 6] = np.where(ref["hit"] == 1, ref["t"], r[:, 6])
    return r, ref["hit"], rng.integers(0, 1 << 20, n).astype(np.int32)


def _soft_by_intersect(o, items, hit, pixels, sl, units, samples, seed, level):
    """lit[i, l] from the oracle's closest hit on every sample ray (main.cpp:173-199 restated in numpy float32)."""
    pts = (items[:, 0:3] + items[:, 3:6] * items[:, 6:7]).astype(np.float32)
    n, L = len(items), len(sl)
    lit = np.zeros((n, L), np.uint32)
    for l in range(L):
        for smp in range(samples):
            u = units[_unit_index(seed, pixels.astype(np.uint32), level, l, smp, len(units))]
            rp = (sl[l, 0:3] + sl[l, 3] * u).astype(np.float32)
            d = occlfam.normalize(rp - pts)
            org = (pts + np.float32(0.001) * d).astype(np.float32)
            lightT = occlfam.length(org - rp)
            ray = np.concatenate([org, d, lightT[:, None]], 1).astype(np.float32)
            ref = o.intersect(ray)
            lit[:, l] += ((ref["hit"] == 0) | (ref["t"] > lightT)).astype(np.uint32)
    lit[hit == 0] = 0
    return lit


def _with_spheres(pkg, sd):
    sph = np.float32([[0.1, -0.2, 0.0, 0.25, -1], [-0.3, 0.35, 0.1, 0.12, -1]])
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials, spheres=sph,
                                point_lights=sd.point_lights)


def test_soft_lit_agrees_with_intersect_on_the_sample_rays(pkg, orc, scene_data):
    sd = _with_spheres(pkg, scene_data("cornell"))
    o = orc.OracleScene(sd)
    items, hit, pixels = _items(pkg, orc, sd, o)
    sl = np.concatenate([pkg.scenes.CORNELL_SPHERICAL_LIGHTS, np.float32([[0.1, -0.2, 0.0, 0.1, 1, 1, 1]]),  # inside a sphere
                         np.float32([[0.0, -0.9, 0.0, 0.2, 1, 1, 1]])])  # below the floor
    units = pkg.unit_vector_table(97, 5)
    for level, seed in ((0, 0), (1, 12345)):
        want = _soft_by_intersect(o, items, hit, pixels, sl, units, 6, seed, level)
        got = o.soft_lit(items, sl, units, 6, seed=seed, level=level, pixels=pixels, hit=hit)
        assert got.shape == (len(items), len(sl)) and np.array_equal(got, want)
        assert 0 < got.sum() < 6 * got.size  # lit and blocked samples both occur
    assert (hit == 0).any() and (hit == 1).any()


def test_soft_lit_O0_equals_O2(pkg, orc, scene_data):
    sd = _with_spheres(pkg, scene_data("cornell"))
    o2, o0 = orc.OracleScene(sd), orc.OracleScene(sd, o0=True)
    items, hit, pixels = _items(pkg, orc, sd, o2, n=200, seed=9)
    sl = pkg.scenes.CORNELL_SPHERICAL_LIGHTS
    units = pkg.unit_vector_table(4096, 1)
    a = o2.soft_lit(items, sl, units, 16, seed=7, level=2, pixels=pixels, hit=hit)
    b = o0.soft_lit(items, sl, units, 16, seed=7, level=2, pixels=pixels, hit=hit)
    assert np.array_equal(a, b) and a.sum() > 0


def test_soft_lit_is_what_shading_counts(pkg, orc, scene_data):
    """shading() divides soft_lit's count by the sample count: a white diffuse-only surface under one white spherical light shades to
    dif * count / samples -- the same loop, not a second statement of it."""
    sd = scene_data("cornell")
    o = orc.OracleScene(sd)
    W, H = 16, 12
    rays = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    ref = o.intersect(rays)
    sl = pkg.scenes.CORNELL_SPHERICAL_LIGHTS[:1]
    units = pkg.unit_vector_table(512, 2)
    rgb, _ = o.shade_rays(rays, np.zeros((0, 6), np.float32), sl, units, samples=9, seed=4, max_level=1)
    items = rays.copy()
    items[:, 6] = np.where(ref["hit"] == 1, ref["t"], items[:, 6])
    lit = o.soft_lit(items, sl, units, 9, seed=4, level=0, hit=ref["hit"])
    dark = ref["hit"] == 1
    assert np.array_equal(rgb[dark & (lit[:, 0] == 0)], np.zeros(((dark & (lit[:, 0] == 0)).sum(), 3), np.float32))
    assert ((rgb.sum(1) > 0) <= (lit[:, 0] > 0)).all()  # light only where some sample got through
    assert (lit[dark, 0] > 0).any() and (lit[dark, 0] < 9).any()


def test_boundary_family_straddles_the_threshold(pkg, orc, scene_data):
    """dist = fl(t + 0.001f) is the last distance at which the closest hit does NOT shadow: one ulp more and it does."""
    sd = scene_data("monkey")
    o = orc.OracleScene(sd)
    rng = np.random.default_rng(1)
    rays = occlfam.aimed_rays(sd, 400, rng)
    ref = o.intersect(rays)
    r = rays[ref["hit"] == 1]
    t = ref["t"][ref["hit"] == 1]
    th = (t + np.float32(0.001)).astype(np.float32)
    assert not occlfam.verdict(1, t, th).any()
    assert occlfam.verdict(1, t, occlfam.ulps(th, 1)).all()
    br, bd = occlfam.boundary(o, r)
    v, _ = occlfam.reference(o, br, bd)
    assert 0 < v.sum() < len(v)


def test_spawn_matches_the_oracle_shadow_ray(pkg, orc):
    """occlfam.spawn restates pointInShadow's ray (main.cpp:104-111): origin += 0.001f * normalize(toLight), dist = |toLight|; a light
    at the point gives a NaN direction and dist 0."""
    pts = np.float32([[0.25, -0.5, 1.0], [3.0, 2.0, 1.0]])
    lights = np.float32([[0.0, 0.58, 0.0], [3.0, 2.0, 1.0]])
    rays, dist = occlfam.spawn(pts, lights)
    to = (lights[0] - pts[0]).astype(np.float32)
    inv = np.float32(1.0) / np.sqrt((to[0] * to[0] + to[1] * to[1]) + to[2] * to[2])
    d = (to * inv).astype(np.float32)
    assert np.array_equal(rays[0, 3:6], d) and np.array_equal(rays[0, 0:3], (pts[0] + np.float32(0.001) * d).astype(np.float32))
    assert rays[0, 6] == occlfam.FMAX and dist[0] == np.sqrt((to[0] * to[0] + to[1] * to[1]) + to[2] * to[2])
    assert np.isnan(rays[3, 3:6]).all() and dist[3] == 0.0

"""GPU: the visibility queries (cgrt_occluded*, cgrt_in_shadow*, cgrt_soft_lit*, include/cgrt.h), every answer
exact against the CPU oracle.

* Any-hit rays: occluded == OracleScene.intersect(rays).hit for ray families (tests/rayfam.py), camera rays, random segments with
  finite t, t set exactly to a hit's t and +-1 ulp (the `t >= ray.t` rule), non-finite rays; in every kernel shape, both walks.
* Point-light shadows: in_shadow == occlfam.verdict(oracle closest hit of occlfam.spawn(points, lights)) for hit points, points on
  walls, inside spheres, a light at the point, scaled scenes and non-finite points; 1, 3 and 7 lights; every shape, both walks.
* Soft shadows: soft_lit == OracleScene.soft_lit of items (origin = point, direction 0, t 0, pixel = index, level 0); any-hit ==
  closest-hit; equal to cgrt_debug_soft_lit on the level-0 hits of a ray list.
* Device, tensor and C++ mirror forms are byte-identical to the host forms; a side stream without synchronise; four threads at once.
* Edges (n == 0, zero lights) and a predicted frame rendered before and after a batch of queries is unchanged."""
import os
import sys
import threading
import zlib

import numpy as np
import pytest

import rayfam

try:  # (imported before libcgrt.so loads, as the other tensor tests do: the process must map torch's HIP runtime only)
    import torch
except ImportError:  # pragma: no cover
    torch = None

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import occlfam  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (-1, 0, 1, 2, 3)  # cgrt_set_kernel_shape: auto, LANE64, QUAD16, LANE16, QUAD4
FMAX = np.finfo(np.float32).max
SPHERES_CORNELL = np.float32([[0.0, 0.3, 0.0, 0.1, -1], [0.25, -0.2, 0.1, 0.15, -1], [-0.3, 0.1, -0.2, 0.08, -1]])


def _with(pkg, sd, spheres=None, lights=None):
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials,
                                spheres=sd.spheres if spheres is None else spheres, point_lights=sd.point_lights if lights is None else lights)


def _scene(pkg, sd):
    pkg.set_fast_tree(1)
    try:
        return pkg.Scene(sd)
    finally:
        pkg.set_fast_tree(-1)


def _walks_and_shapes(pkg, sc):
    """(walk, shape) for both walks (when the scene has a fast tree) and every kernel shape; restores the defaults."""
    walk0 = sc.walk()
    try:
        for walk in ((True, False) if walk0 else (False,)):
            sc.set_walk(walk)
            for shape in SHAPES:
                pkg.set_kernel_shape(shape)
                yield walk, shape
    finally:
        pkg.set_kernel_shape(-1)
        sc.set_walk(bool(walk0))


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    out = {"cube": scene_data("cube"), "cornell": scene_data("cornell"), "monkey": scene_data("monkey"), "blob": scene_data("blob")}
    out["cornell_spheres"] = _with(pkg, out["cornell"], spheres=SPHERES_CORNELL)
    out["spheres"] = _with(pkg, scene_data("spheres"), lights=np.float32([[3, 0, 3, 15, 15, 15], [0, 0, 6, 1, 1, 1], [0, 0, 20, 1, 1, 1]]))
    out["dragon"] = pkg.scenes.make_dragon(40_000)
    out["dragon"].point_lights = np.float32([[0.0, 2.0, -2.0, 1, 1, 1]])
    out["cube_2^30"] = occlfam.scaled(out["cube"], 2.0**30, pkg)
    out["blob_2^-20"] = occlfam.scaled(out["blob"], 2.0**-20, pkg)
    return out


# ---- any-hit rays ----
def _occlusion_rays(pkg, orc, sd, rng):
    W, H = 48, 32
    cam = orc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    o = orc.OracleScene(sd)
    parts = [cam, occlfam.aimed_rays(sd, 400, rng)]
    if len(sd.tri):
        _, boxes = o.nodes()
        fam = rayfam.families(sd, boxes, cam[:200], rng=np.random.RandomState(rng.integers(1 << 30)), n_random=300)
        parts.append(rayfam.concat(fam))
        parts.append(rayfam.arbitrary_rays(sd, 600, int(rng.integers(1 << 30)))[0])
    base = np.concatenate(parts).astype(np.float32)
    # segments: finite t, and t at a hit's t and one ulp either side (a hit at exactly ray.t is not taken: `t >= ray.t`)
    ref = o.intersect(base)
    m = ref["hit"] == 1
    seg = base[m].copy()
    t = ref["t"][m]
    segs = []
    for k in (-1, 0, 1):
        s = seg.copy()
        s[:, 6] = occlfam.ulps(t, k)
        segs.append(s)
    r = base[rng.permutation(len(base))[:800]].copy()
    r[:, 6] = rng.uniform(0.0, 3.0, len(r)).astype(np.float32) * np.abs(r[:, 0:3]).max()
    segs.append(r)
    nf = base[:64].copy()
    nf[0:8, 0] = np.nan
    nf[8:16, 3] = np.nan
    nf[16:24, 4] = np.inf
    nf[24:32, 1] = -np.inf
    nf[32:40, 6] = np.nan
    nf[40:48, 6] = np.inf
    nf[48:56, 3:6] = 0.0
    nf[56:64, 6] = 0.0
    rays = np.ascontiguousarray(np.concatenate([base] + segs + [nf]).astype(np.float32))
    return rays, o.intersect(rays)["hit"] == 1


@pytest.mark.parametrize("name", ["cube", "cornell", "cornell_spheres", "spheres", "monkey", "dragon", "cube_2^30", "blob_2^-20"])
def test_occluded_matches_oracle(pkg, orc, scenes, name):
    sd = scenes[name]
    rays, want = _occlusion_rays(pkg, orc, sd, np.random.default_rng(zlib.crc32(name.encode())))
    assert 0 < want.sum() < len(want)
    sc = _scene(pkg, sd)
    try:
        for walk, shape in _walks_and_shapes(pkg, sc):
            got = sc.occluded(rays)
            assert got.dtype == np.bool_ and got.shape == want.shape
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"{name} walk {walk} shape {shape}: {len(bad)} of {len(want)} differ, first {bad[:5].tolist()}"
            hits, _ = sc.intersect(rays, want_normals=False)
            assert np.array_equal(got, hits["hit"] == 1), "occluded != the closest hit's flag"
    finally:
        sc.close()


def test_occluded_equals_intersect_on_the_dragon_1080p(pkg):
    sd = pkg.scenes.make_dragon(800_000)
    W, H = 1920, 1080
    sc = pkg.Scene(sd)
    try:
        rays = sc.generate_rays(pkg.scenes.default_camera(W, H), W, H).view(np.float32).reshape(-1, 7).copy()
        rng = np.random.default_rng(5)
        rays[:, 6] = rng.uniform(0.5, 4.0, len(rays)).astype(np.float32)  # finite segments: some end before the surface
        hits, _ = sc.intersect(rays, want_normals=False)
        got = sc.occluded(rays)
        assert 0 < got.sum() < len(got)
        assert np.array_equal(got, hits["hit"] == 1)
    finally:
        sc.close()


# ---- point-light shadows ----
def _shadow_points(pkg, orc, sd, rng):
    o = orc.OracleScene(sd)
    W, H = 40, 30
    base = np.concatenate([orc.generate_rays(pkg.scenes.default_camera(W, H), W, H), occlfam.aimed_rays(sd, 400, rng)])
    pts, _, _ = occlfam.hit_points(o, base)
    pts = pts[rng.permutation(len(pts))[:700]]
    parts = [pts]
    if len(sd.tri):  # on the walls: origins of occlfam.on_walls' rays
        wr, _ = occlfam.on_walls(sd, 200, rng)
        parts.append(wr[:, 0:3])
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 5)
    if len(sph):  # inside spheres
        u = occlfam.normalize(rng.normal(size=(len(sph), 8, 3)).astype(np.float32))
        parts.append((sph[:, None, 0:3] + sph[:, None, 3:4] * np.float32(0.5) * u).reshape(-1, 3))
    nf = pts[:6].copy()
    nf[0, 0], nf[1, 1], nf[2, 2], nf[3] = np.nan, np.inf, -np.inf, np.nan
    nf[4] = FMAX
    parts.append(nf)
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


def _lights(sd, pts, k, rng):
    """k lights: the scene's, random ones about it, one at a hit point (a light AT some point) and one 2 ulps off another."""
    L = [np.asarray(sd.point_lights, np.float32).reshape(-1, 6)]
    lo, hi = np.nanmin(pts[np.isfinite(pts).all(1)], 0), np.nanmax(pts[np.isfinite(pts).all(1)], 0)
    c, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, np.float32(1e-30))
    L.append(np.concatenate([pts[:1], np.ones((1, 3), np.float32)], 1))
    L.append(np.concatenate([occlfam.ulps(pts[1:2], 2), np.ones((1, 3), np.float32)], 1))
    rnd = (c + rng.uniform(-1.6, 1.6, (8, 3)) * ext).astype(np.float32)
    L.append(np.concatenate([rnd, np.ones((8, 3), np.float32)], 1))
    return np.ascontiguousarray(np.concatenate(L)[:k].astype(np.float32))


@pytest.mark.parametrize("name", ["cube", "cornell", "cornell_spheres", "spheres", "dragon", "cube_2^30", "blob_2^-20"])
def test_in_shadow_matches_oracle(pkg, orc, scenes, name):
    sd = scenes[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 0x5A)
    pts = _shadow_points(pkg, orc, sd, rng)
    o = orc.OracleScene(sd)
    sc = _scene(pkg, sd)
    try:
        for k in (1, 3, 7):
            lights = _lights(sd, pts, k, rng)
            rays, dist = occlfam.spawn(pts, lights[:, 0:3])
            want = occlfam.reference(o, rays, dist)[0].reshape(len(pts), len(lights))
            for walk, shape in _walks_and_shapes(pkg, sc):
                got = sc.in_shadow(pts, lights)
                bad = np.argwhere(got != want)
                assert len(bad) == 0, f"{name} lights {k} walk {walk} shape {shape}: {len(bad)} differ, first {bad[:5].tolist()}"
    finally:
        sc.close()


def test_in_shadow_boundary_distances(pkg, orc, scenes):
    """A light exactly at an occluder's hit distance + 0.001f, and 2 ulps either side: the verdict flips where the reference's does."""
    sd = scenes["cornell"]
    o = orc.OracleScene(sd)
    rng = np.random.default_rng(11)
    pts, _, _ = occlfam.hit_points(o, occlfam.aimed_rays(sd, 300, rng))
    lights = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    rays, dist = occlfam.spawn(pts, lights[:, 0:3])
    ref = o.intersect(rays)
    m = ref["hit"] == 1
    assert m.any()
    # move each light along its ray so that |fromPosToLight| lands near the hit's t + 0.001f
    sc = _scene(pkg, sd)
    try:
        for k in (-2, -1, 0, 1, 2):
            d = rays[m, 3:6]
            tgt = occlfam.ulps((ref["t"][m] + np.float32(0.001)).astype(np.float32), k)
            lp = (pts[np.flatnonzero(m) // len(lights)] + d * tgt[:, None]).astype(np.float32)
            for j in range(0, len(lp), 64):
                L = np.concatenate([lp[j : j + 64], np.ones((len(lp[j : j + 64]), 3), np.float32)], 1)
                P = pts[np.flatnonzero(m)[j : j + 64] // len(lights)]
                r2, d2 = occlfam.spawn(P, L[:, 0:3])
                want = occlfam.reference(o, r2, d2)[0].reshape(len(P), len(L))
                assert np.array_equal(sc.in_shadow(P, L), want), f"boundary offset {k} ulps, block {j}"
    finally:
        sc.close()


# ---- soft shadows ----
def _soft_setup(pkg, sd):
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3]
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 5)
    pts = np.concatenate([p, sph[:, :3]]) if len(p) else sph[:, :3]
    lo, hi = pts.min(0), pts.max(0)
    c, ext = (lo + hi) / 2, (hi - lo) / 2
    r = np.float32(0.05) * ext.max()
    sl = [[*(c + np.float32([0, 0.8, 0]) * ext), r, 1, 1, 1], [*(c + np.float32([0.3, -0.9, 0.2]) * ext), r, 1, 1, 1]]
    for s in sph[:2]:
        sl.append([*s[:3], s[3] * np.float32(0.5), 1, 1, 1])
    return np.asarray(sl, np.float32), pkg.unit_vector_table(1000, 3)


def _no_negative_zero(p):
    p = p.copy()
    p[(p == 0) & np.signbit(p)] = np.float32(0.0)
    return p


@pytest.mark.parametrize("name", ["cornell", "cornell_spheres", "spheres", "dragon"])
def test_soft_lit_matches_oracle(pkg, orc, scenes, name):
    sd = scenes[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) ^ 0x50F7)
    o = orc.OracleScene(sd)
    pts, _, _ = occlfam.hit_points(o, occlfam.aimed_rays(sd, 700, rng))
    pts = _no_negative_zero(pts)
    sl, units = _soft_setup(pkg, sd)
    samples, seed = 8, 77
    items = np.zeros((len(pts), 7), np.float32)
    items[:, 0:3] = pts  # origin = p, direction 0, t 0: pointOn = p + 0 * 0 = p
    want = o.soft_lit(items, sl, units, samples, seed=seed, level=0, pixels=np.arange(len(pts), dtype=np.int32), hit=np.ones(len(pts), np.uint32))
    assert 0 < want.sum() < want.size * samples
    sc = _scene(pkg, sd)
    try:
        for walk in ((True, False) if sc.walk() else (False,)):
            sc.set_walk(walk)
            for closest in (False, True):
                got = sc.soft_lit(pts, sl, units, samples=samples, seed=seed, closest_hit=closest)
                assert got.dtype == np.uint32 and got.shape == want.shape
                bad = np.argwhere(got != want)
                assert len(bad) == 0, f"{name} walk {walk} closest {closest}: {len(bad)} differ, first {bad[:5].tolist()}"
    finally:
        sc.close()


def test_soft_lit_equals_the_frames_counts(pkg, orc, scenes):
    """The level-0 hits of a ray list: cgrt_soft_lit of their points == cgrt_debug_soft_lit (the frame's launcher) on the same items
    sampled as pixel i, level 0 -- the counts cgrt_shade_rays uses."""
    sd = scenes["cornell_spheres"]
    rng = np.random.default_rng(3)
    rays = occlfam.aimed_rays(sd, 900, rng)
    sc = pkg.Scene(sd)
    try:
        hits, _ = sc.intersect(rays, want_normals=False)
        m = hits["hit"] == 1
        r, h = np.ascontiguousarray(rays[m]), np.ascontiguousarray(hits[m])
        pts = (r[:, 0:3] + r[:, 3:6] * h["t"][:, None]).astype(np.float32)
        sl, units = _soft_setup(pkg, sd)
        want = sc.debug_soft_lit(r, h, np.arange(len(r), dtype=np.int32), sl, units, 16, seed=9, level=0, anyhit=True)
        assert np.array_equal(sc.soft_lit(pts, sl, units, samples=16, seed=9), want)
    finally:
        sc.close()


# ---- device, tensor and mirror forms; streams; threads ----
@pytest.fixture(scope="module")
def cornell_case(pkg, orc, scenes):
    sd = scenes["cornell_spheres"]
    rng = np.random.default_rng(21)
    rays, _ = _occlusion_rays(pkg, orc, sd, rng)
    pts = _no_negative_zero(_shadow_points(pkg, orc, sd, rng))
    lights = _lights(sd, pts, 3, rng)
    sl, units = _soft_setup(pkg, sd)
    return sd, rays, pts, lights, sl, units


def test_device_and_tensor_forms_equal_host_forms(pkg, cornell_case):
    if torch is None:
        pytest.skip("torch is not installed")
    sd, rays, pts, lights, sl, units = cornell_case
    sc = pkg.Scene(sd)
    try:
        occ, sh, lit = sc.occluded(rays), sc.in_shadow(pts, lights), sc.soft_lit(pts, sl, units, samples=8, seed=4)
        dev = torch.device("cuda", 0)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):  # inputs written on the side stream and queried on it, no synchronise in between
            tr = torch.empty(rays.shape, dtype=torch.float32, device=dev)
            tp = torch.empty(pts.shape, dtype=torch.float32, device=dev)
            tr.copy_(torch.from_numpy(rays), non_blocking=False)
            tp.copy_(torch.from_numpy(pts), non_blocking=False)
            tr.mul_(1.0)
            tp.mul_(1.0)
            a = sc.occluded_tensor(tr, stream=side)
            b = sc.in_shadow_tensor(tp, lights=lights, stream=side)
            c = sc.soft_lit_tensor(tp, sl, units, samples=8, seed=4, stream=side)
            o8 = torch.full((len(rays),), 7, dtype=torch.uint8, device=dev)
            sc.occluded_tensor(tr, out=o8, stream=side)
        side.synchronize()
        assert a.dtype == torch.bool and b.dtype == torch.bool and c.dtype == torch.int32
        assert tuple(b.shape) == (len(pts), len(lights)) and tuple(c.shape) == (len(pts), len(sl))
        assert np.array_equal(a.cpu().numpy(), occ) and np.array_equal(o8.cpu().numpy(), occ.view(np.uint8))
        assert np.array_equal(b.cpu().numpy(), sh)
        assert np.array_equal(c.cpu().numpy().view(np.uint32), lit)
        # shapes (..., 7) / (..., 3)
        pts4 = tp[: (len(pts) // 4) * 4].view(-1, 4, 3)
        assert np.array_equal(sc.in_shadow_tensor(pts4, lights=lights).cpu().numpy().reshape(-1, len(lights)), sh[: len(pts4) * 4])
        # raw device pointers
        hb = torch.zeros(len(rays), dtype=torch.uint8, device=dev)
        sc.occluded_device(tr.data_ptr(), len(rays), hb.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(hb.cpu().numpy(), occ.view(np.uint8))
        # out validation happens before any call
        for bad in (torch.zeros(len(rays) + 1, dtype=torch.bool, device=dev), torch.zeros(len(rays), dtype=torch.int32, device=dev),
                    torch.zeros(len(rays), dtype=torch.bool)):
            with pytest.raises(ValueError):
                sc.occluded_tensor(tr, out=bad)
        with pytest.raises(ValueError):
            sc.soft_lit_tensor(tp, sl, units, out=torch.zeros((len(pts), len(sl)), dtype=torch.uint8, device=dev))
        # empty inputs
        assert sc.occluded_tensor(tr[:0]).shape == (0,)
        assert tuple(sc.in_shadow_tensor(tp[:0], lights=lights).shape) == (0, len(lights))
    finally:
        sc.close()


def test_mirror_equals_c_abi(pkg, scenes):
    sd = scenes["cornell"]  # (the mirror's flat-array scenes carry no spheres)
    rng = np.random.default_rng(8)
    rays = occlfam.aimed_rays(sd, 500, rng)
    rays[::3, 6] = rng.uniform(0.1, 2.0, len(rays[::3])).astype(np.float32)
    sc = pkg.Scene(sd)
    try:
        hits, _ = sc.intersect(rays, want_normals=False)
        m = hits["hit"] == 1
        pts = _no_negative_zero((rays[m, 0:3] + rays[m, 3:6] * hits["t"][m][:, None]).astype(np.float32))
        sl, units = _soft_setup(pkg, sd)
        assert np.array_equal(pkg.host_occluded(sd, rays), sc.occluded(rays))
        assert np.array_equal(pkg.host_in_shadow(sd, pts), sc.in_shadow(pts))
        assert np.array_equal(pkg.host_soft_lit(sd, pts, sl, units, samples=8, seed=2), sc.soft_lit(pts, sl, units, samples=8, seed=2))
    finally:
        sc.close()


def test_four_threads_query_one_scene(pkg, cornell_case):
    sd, rays, pts, lights, sl, units = cornell_case
    sc = pkg.Scene(sd)
    try:
        want = (sc.occluded(rays), sc.in_shadow(pts, lights), sc.soft_lit(pts, sl, units, samples=8))
        got, errors = [None] * 4, []

        def work(k):
            try:
                r = []
                for _ in range(5):
                    r.append((sc.occluded(rays), sc.in_shadow(pts, lights), sc.soft_lit(pts, sl, units, samples=8)))
                got[k] = r
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        for r in got:
            for a, b, c in r:
                assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(c, want[2])
    finally:
        sc.close()


# ---- edges, and existing behaviour ----
def test_edges(pkg, cornell_case):
    sd, rays, pts, lights, sl, units = cornell_case
    sc = pkg.Scene(sd)
    try:
        assert sc.occluded(np.zeros((0, 7), np.float32)).shape == (0,)
        assert sc.in_shadow(np.zeros((0, 3), np.float32), lights).shape == (0, len(lights))
        assert sc.in_shadow(pts, np.zeros((0, 6), np.float32)).shape == (len(pts), 0)
        assert sc.soft_lit(np.zeros((0, 3), np.float32), sl, units).shape == (0, len(sl))
        assert sc.soft_lit(pts, np.zeros((0, 7), np.float32), units).shape == (len(pts), 0)
        assert sc.soft_lit(pts[:3], sl, units, samples=1 << 24).max() <= 1 << 24
        # a list across the kernel-shape thresholds (8192, 131072) and an odd length
        big = np.ascontiguousarray(np.resize(rays, (131073, 7)))
        want = sc.intersect(big, want_normals=False)[0]["hit"] == 1
        assert np.array_equal(sc.occluded(big), want)
        assert np.array_equal(sc.occluded(big[:8193]), want[:8193])
    finally:
        sc.close()


def test_frames_unchanged_by_queries(pkg, cornell_case):
    sd, rays, pts, lights, sl, units = cornell_case
    W, H = 96, 64
    cam = pkg.scenes.default_camera(W, H)
    sc = pkg.Scene(sd)
    try:
        pkg.set_render_prediction(True)
        a0, _ = sc.render(cam, W, H)
        a1, _ = sc.render(cam, W, H)  # predicted
        assert sc.last_render_path() == 1
        hints_before = sc.hint_counts()
        t0, _ = sc.trace_primary(cam, W, H)
        sc.occluded(rays)
        sc.in_shadow(pts, lights)
        sc.soft_lit(pts, sl, units, samples=8)
        b1, _ = sc.render(cam, W, H)
        assert sc.last_render_path() == 1, "the prediction record survived the queries"
        assert np.array_equal(a1.view(np.uint32), b1.view(np.uint32)) and np.array_equal(a0.view(np.uint32), b1.view(np.uint32))
        assert np.array_equal(sc.trace_primary(cam, W, H)[0].view(np.uint8), t0.view(np.uint8))
        assert sc.hint_counts() == hints_before
    finally:
        sc.close()

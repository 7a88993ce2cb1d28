"""Shadow verdicts and soft-shadow counts of the shipped occlusion launchers against the CPU oracle, ray by ray.

A shaded frame hides most wrong shadow verdicts: an unoccluded point light adds dif + spec, and both are zero for a light behind the
surface, for black materials or lights (k_shade), so only the verdicts themselves can show a fault.  cgrt_debug_trace_shadow and
cgrt_debug_soft_lit run the frame's own launchers (launch_trace_shadow, launch_trace_pair, launch_soft_shadow) on caller rays:
  * point-light shadow rays: `hit && !(t + 0.001f >= dist)` from the device hit equals the same test on the oracle's closest hit,
    for every ray, on every path -- (a) n known on the host; (b) the length in a device word x dmul, the grid for a larger capacity,
    the host's estimate missing, too small or too large; (c) the pair launch beside a mirror list (whose closest hits are checked
    too), shadow-to-mirror 1:0, 1:1, 1:7, 7:1 -- in every kernel shape, on the certified and the exact walk, with the fast tree built
    and not built.  Entries past the list keep the call's 0xA5 fill: a ray the kernel skipped or wrote twice cannot pass as a miss;
  * spherical lights: the integer count per (item, light), closest-hit and any-hit sample rays, against OracleScene.soft_lit.
Ray families (tools/occlfam.py): shadow rays spawned from real hits towards the scenes' lights, random lights, lights behind the
surface, on it (zero direction, dist 0), inside closed meshes; the epsilon boundary (dist = fl(t + 0.001f) +-2 ulps) and dist between
two layers' thresholds (dragon, blob, stacked plates); origins on axis-aligned walls, directions along them; duplicated triangles
(ties); scales 2^-20 .. 2^37 (at 2^30 and above the 0.001 offset rounds away and the origin stays on the surface); spheres in front of
and behind lights, origins inside spheres, a spheres-only scene; NaN / infinite / zero dist and zero or NaN directions."""
import os
import sys
import time
import zlib

import numpy as np
import pytest
from conftest import same_bits

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import occlfam  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = (-1, 0, 1, 2, 3)  # cgrt_set_kernel_shape: auto, LANE64, QUAD16, LANE16, QUAD4
PAIR_SHAPES = (-1, 0, 2)  # can_trace_pair: the lane shapes only
RATIOS = ((1, 0), (1, 1), (1, 7), (7, 1))  # shadow : mirror rays of a pair launch
MAX_RAYS = 6000  # per case (a multiple of 6: dmul 2 and 3 divide it)
SPHERES_CORNELL = np.float32([[0.0, 0.3, 0.0, 0.1, -1],  # between the floor and the ceiling light
                              [0.25, -0.2, 0.1, 0.15, -1], [-0.3, 0.1, -0.2, 0.08, -1]])
SCALES = (-20, -7, 10, 30, 37)


def _with(pkg, sd, spheres=None, lights=None):
    return pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=sd.materials,
                                spheres=sd.spheres if spheres is None else spheres, point_lights=sd.point_lights if lights is None else lights)


def _case(pkg, orc, name, sd, base, rng, extra_lights=(), walls=False, inside=None):
    """The case's shadow rays (n a multiple of 6) and dist, the oracle's verdicts and closest hits."""
    o = orc.OracleScene(sd)
    sr, sdist = occlfam.spawned(o, sd, base, rng, extra_lights=extra_lights, max_points=500)
    parts = [(sr, sdist)]
    pick = rng.choice(len(sr), min(len(sr), 600), replace=False) if len(sr) else np.zeros(0, np.int64)
    parts.append(occlfam.boundary(o, np.concatenate([sr[pick], base[:400]]), rng=rng, max_rays=500))
    parts.append(occlfam.nonfinite(sr[rng.permutation(len(sr))], sdist))
    if walls:
        parts.append(occlfam.on_walls(sd, 300, rng))
    if inside is not None:  # origins inside spheres (centre + some way out), towards the lights
        c = np.asarray(inside, np.float32).reshape(-1, 5)
        pts = (c[:, None, 0:3] + c[:, None, 3:4] * np.float32(0.5) * occlfam.normalize(rng.normal(size=(len(c), 8, 3)).astype(np.float32)))
        lp = np.concatenate([np.asarray(sd.point_lights, np.float32).reshape(-1, 6)[:, :3], np.asarray(extra_lights, np.float32).reshape(-1, 3)])
        parts.append(occlfam.spawn(pts.reshape(-1, 3).astype(np.float32), lp))
    rays = np.concatenate([p[0] for p in parts]).astype(np.float32)
    dist = np.concatenate([p[1] for p in parts]).astype(np.float32)
    k = rng.permutation(len(rays))[:MAX_RAYS]
    k = k[: len(k) // 6 * 6]
    rays, dist = np.ascontiguousarray(rays[k]), np.ascontiguousarray(dist[k])
    want, ref = occlfam.reference(o, rays, dist)
    return dict(name=name, sd=sd, rays=rays, dist=dist, want=want, ref=ref)


@pytest.fixture(scope="module")
def cases(pkg, orc, scene_data):
    rng = np.random.default_rng(0x0CC1)
    out = {}
    W, H = 40, 30

    def cam_rays(n_aim, sd):
        return np.concatenate([orc.generate_rays(pkg.scenes.default_camera(W, H), W, H), occlfam.aimed_rays(sd, n_aim, rng)])

    cube = scene_data("cube")
    out["cube"] = _case(pkg, orc, "cube", cube, cam_rays(300, cube), rng, extra_lights=[[0.5, 0.5, 0.5]])  # inside the closed cube
    cornell = scene_data("cornell")
    out["cornell"] = _case(pkg, orc, "cornell", cornell, cam_rays(300, cornell), rng, walls=True)
    cs = _with(pkg, cornell, spheres=SPHERES_CORNELL)
    out["cornell_spheres"] = _case(pkg, orc, "cornell_spheres", cs, cam_rays(300, cs), rng, extra_lights=[[0.0, 0.3, 0.0], [0.0, 0.1, 0.0]],
                                   inside=SPHERES_CORNELL)
    out["cornell_dup"] = _case(pkg, orc, "cornell_dup", occlfam.duplicated(cornell, pkg), cam_rays(300, cornell), rng, walls=True)
    for name in ("monkey", "dodge"):
        sd = scene_data(name)
        out[name] = _case(pkg, orc, name, sd, cam_rays(300, sd), rng)
    blob = scene_data("blob")
    out["blob"] = _case(pkg, orc, "blob", blob, cam_rays(300, blob), rng, extra_lights=[[0.0, 0.0, 0.0]])
    sph = scene_data("spheres")
    sph = _with(pkg, sph, lights=np.float32([[3, 0, 3, 15, 15, 15], [0, 0, 6, 1, 1, 1], [0, 0, 20, 1, 1, 1]]))  # inside a sphere, behind all
    base = np.concatenate([occlfam.aimed_rays(sph, 600, rng), occlfam.aimed_rays(sph, 300, rng, origin=(0.0, 0.0, 0.0))])
    out["spheres"] = _case(pkg, orc, "spheres", sph, base, rng, inside=sph.spheres)
    dragon = pkg.scenes.make_dragon(40_000)
    dragon.point_lights = np.float32([[0.0, 2.0, -2.0, 1, 1, 1]])
    out["dragon"] = _case(pkg, orc, "dragon", dragon, cam_rays(600, dragon), rng)
    pl = occlfam.plates(pkg)
    up = occlfam.aimed_rays(pl, 600, rng, origin=(0.05, -0.1, -0.5))
    out["plates"] = _case(pkg, orc, "plates", pl, up, rng, extra_lights=[[0.0, 0.0, 0.2], [0.3, 0.1, 0.055]])
    for e in SCALES:
        for name, sd0 in (("cube", cube), ("blob", blob)):
            sd = occlfam.scaled(sd0, 2.0**e, pkg)
            out[f"{name}_2^{e}"] = _case(pkg, orc, f"{name}_2^{e}", sd, occlfam.aimed_rays(sd, 500, rng), rng)
    return out


def _fill_ok(h):
    return (h.view(np.uint8) == 0xA5).all()


def _check(c, got, n, cap, tag):
    h = got[:n]
    assert np.isin(h["hit"], (0, 1)).all(), f"{c['name']} {tag}: rays the kernel did not write: {np.nonzero(~np.isin(h['hit'], (0, 1)))[0][:10]}"
    v = occlfam.verdict(h["hit"], h["t"], c["dist"][:n])
    bad = np.nonzero(v != c["want"][:n])[0]
    assert len(bad) == 0, (f"{c['name']} {tag}: {len(bad)} of {n} verdicts differ, first {bad[:8]}: device hit/t {h['hit'][bad[:4]]} "
                           f"{h['t'][bad[:4]]}, oracle {c['ref']['hit'][bad[:4]]} {c['ref']['t'][bad[:4]]}, dist {c['dist'][bad[:4]]}")
    assert _fill_ok(got[n:cap]), f"{c['name']} {tag}: entries past the list were written"


def _mirror(c, k):
    """k mirror rays (closest-hit queries) from the case's rays, tiled; with the oracle's answer."""
    idx = np.arange(k) % max(1, len(c["rays"]))
    return np.ascontiguousarray(c["rays"][idx]), c["ref"][idx]


def _check_mirror(c, mh, mn, want, m, mcap, tag):
    h = mh[:m]
    assert np.array_equal(h["hit"], want["hit"]), f"{c['name']} {tag}: mirror hit flags differ"
    hit = want["hit"] == 1
    assert same_bits(h["t"][hit], want["t"][hit]).all() and np.array_equal(h["prim_id"][hit], want["prim"][hit]), f"{c['name']} {tag}: mirror t / prim"
    assert np.array_equal(h["material_id"][hit], want["material"][hit]), f"{c['name']} {tag}: mirror material"
    assert same_bits(mn[:m][hit], want["normal"][hit]).all(), f"{c['name']} {tag}: mirror normals"
    assert _fill_ok(mh[m:mcap]), f"{c['name']} {tag}: mirror entries past the list were written"


def _run_paths(pkg, sc, c, n, shape, pair_ok, tag):
    rays, dist = c["rays"][:n], c["dist"][:n]
    got = sc.debug_trace_shadow(rays, dist, how=0)
    _check(c, got, n, n, f"{tag} (a)")
    for dmul, cap, exp in ((3 if n % 3 == 0 else 1, n + 129, 0), (2 if n % 2 == 0 else 1, 2 * n + 7, max(1, n // 16)),
                           (1, n, 8 * n + 64), (3 if n % 3 == 0 else 1, n + 3, n)):
        got = sc.debug_trace_shadow(rays, dist, how=1, dmul=dmul, capacity=cap, expected=exp)
        _check(c, got, n, max(n, cap), f"{tag} (b) dmul {dmul} capacity {cap} expected {exp}")
    if not pair_ok:  # (c) does not apply: the scene has no fast tree on, or the forced shape is a quad shape
        with pytest.raises(pkg.CgrtError) as ei:
            sc.debug_trace_shadow(rays, dist, how=2, dmul=1, capacity=n)
        assert ei.value.code == -1
        return
    for rs, rm in RATIOS:
        ns = n if rs >= rm else min(n, max(1, n // 7))
        m = ns * rm // rs
        mr, mw = _mirror(c, m)
        dmul = 3 if ns % 3 == 0 else 1
        for exp, mexp in ((0, 0), (ns, m)):
            got, mh, mn = sc.debug_trace_shadow(rays[:ns], dist[:ns], how=2, dmul=dmul, capacity=ns + 64, expected=exp, mirror_rays=mr,
                                                mirror_capacity=m + 65, mirror_expected=mexp)
            t2 = f"{tag} (c) {rs}:{rm} expected {exp}/{mexp}"
            _check(c, got, ns, ns + 64, t2)
            _check_mirror(c, mh, mn, mw, m, m + 65, t2)


def _configs(pkg, sd):
    """(label, scene) for: fast tree built + certified walk, the same scene on the exact walk, no fast tree at all."""
    pkg.set_fast_tree(1)
    try:
        sc = pkg.Scene(sd)
    finally:
        pkg.set_fast_tree(-1)
    out = []
    if sc.walk():
        out.append(("certified", sc))
    pkg.set_fast_tree(0)
    try:
        s0 = pkg.Scene(sd)
    finally:
        pkg.set_fast_tree(-1)
    assert s0.walk() == 0
    return out, sc, s0


CASE_NAMES = ["cube", "cornell", "cornell_spheres", "cornell_dup", "monkey", "dodge", "blob", "spheres", "dragon", "plates"] + [
    f"{n}_2^{e}" for e in SCALES for n in ("cube", "blob")]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_shadow_verdicts_match_oracle(pkg, orc, cases, name):
    c = cases[name]
    t0 = time.time()
    n = len(c["rays"])
    assert n >= 600 and c["want"].any() and (~c["want"]).any(), (name, n)
    certified, sc, s0 = _configs(pkg, c["sd"])
    try:
        for shape in SHAPES:
            pkg.set_kernel_shape(shape)
            if certified:
                sc.set_walk(True)
                _run_paths(pkg, sc, c, n, shape, shape in PAIR_SHAPES, f"certified shape {shape}")
                sc.set_walk(False)
            _run_paths(pkg, sc, c, n, shape, False, f"exact (fast tree built) shape {shape}")
            _run_paths(pkg, s0, c, n, shape, False, f"no fast tree shape {shape}")
    finally:
        pkg.set_kernel_shape(-1)
        sc.close()
        s0.close()
    print(f"{name}: {n} shadow rays, {int(c['want'].sum())} in shadow, certified {bool(certified)}, {time.time() - t0:.1f} s")


def test_certified_walk_falls_back_on_some_shadow_rays(pkg, cases):
    """The path "no certificate, then the exact walk" is exercised by the rays above: count_batch on the same rays (the closest-hit walk,
    whose certificate is the shadow walk's) reports fallback rays on some certified scene, and the fast tree carries most rays."""
    fb = tree = certified = 0
    for name in CASE_NAMES:
        sd = cases[name]["sd"]
        pkg.set_fast_tree(1)
        try:
            sc = pkg.Scene(sd)
        finally:
            pkg.set_fast_tree(-1)
        if sc.walk():
            certified += 1
            cnt = sc.count_batch(cases[name]["rays"])
            fb += cnt["fallback_rays"]
            tree += cnt["tree_rays"]
        sc.close()
    assert certified >= 8 and fb > 0 and tree > fb, (certified, fb, tree)


LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 8191, 8192, 8193, 131071, 131072, 131073, 200_003)


def test_shadow_list_lengths(pkg, orc, cases):
    """Every path at the lengths where the kernel shapes and the device's 16/64-rays-per-wave switch change (the QUAD4 bound 8192, the
    LANE16 bound 131072), on the dragon stand-in's rays tiled to ~200 K."""
    c0 = cases["dragon"]
    N = max(LENGTHS)
    idx = np.arange(N) % len(c0["rays"])
    c = dict(name="dragon tiled", sd=c0["sd"], rays=np.ascontiguousarray(c0["rays"][idx]), dist=np.ascontiguousarray(c0["dist"][idx]),
             want=c0["want"][idx], ref=c0["ref"][idx])
    certified, sc, s0 = _configs(pkg, c["sd"])
    assert certified
    try:
        for n in LENGTHS:
            for shape in SHAPES:
                pkg.set_kernel_shape(shape)
                sc.set_walk(True)
                _run_paths(pkg, sc, c, n, shape, shape in PAIR_SHAPES, f"certified n {n} shape {shape}")
            pkg.set_kernel_shape(-1)
            sc.set_walk(False)
            _run_paths(pkg, sc, c, n, -1, False, f"exact n {n}")
    finally:
        pkg.set_kernel_shape(-1)
        sc.close()
        s0.close()


def _soft_items(orc, o, sd, rng, n):
    rays = np.concatenate([occlfam.aimed_rays(sd, n, rng)])
    rays[::9, 3:6] *= np.float32(-1.0)  # some items missed
    ref = o.intersect(rays)
    items = rays.copy()
    items[:, 6] = np.where(ref["hit"] == 1, ref["t"], items[:, 6])
    hits = np.zeros(n, [("t", np.float32), ("prim_id", np.uint32), ("material_id", np.int32), ("hit", np.uint32)])
    hits["t"], hits["prim_id"], hits["material_id"], hits["hit"] = ref["t"], ref["prim"], ref["material"], ref["hit"]
    return rays, items, hits


@pytest.mark.parametrize("name", ["cornell", "cornell_spheres", "spheres", "dragon", "cube_2^30"])
def test_soft_shadow_counts_match_oracle(pkg, orc, cases, name):
    sd = cases[name]["sd"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    o = orc.OracleScene(sd)
    rays, items, hits = _soft_items(orc, o, sd, rng, 700)
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3]
    sph = np.asarray(sd.spheres, np.float32).reshape(-1, 5)
    pts = np.concatenate([p, sph[:, :3]]) if len(p) else sph[:, :3]
    lo, hi = pts.min(0), pts.max(0)
    c, ext = (lo + hi) / 2, (hi - lo) / 2
    r = np.float32(0.05) * ext.max()
    sl = [[*(c + np.float32([0, 0.8, 0]) * ext), r, 1, 1, 1], [*(c + np.float32([0.3, -0.9, 0.2]) * ext), r, 1, 1, 1]]
    for s in sph[:2]:  # inside a sphere, and just behind one
        sl.append([*s[:3], s[3] * np.float32(0.5), 1, 1, 1])
        sl.append([*(s[:3] + np.float32([0, 0, 1.5]) * s[3]), s[3] * np.float32(0.3), 1, 1, 1])
    sl = np.asarray(sl, np.float32)
    units = pkg.unit_vector_table(1000, 3)
    pixels = rng.integers(0, 1 << 22, len(items)).astype(np.int32)
    samples, seed = 8, 77
    for level in (0, 1):
        want = o.soft_lit(items, sl, units, samples, seed=seed, level=level, pixels=pixels, hit=hits["hit"])
        assert 0 < want.sum() < want.size * samples
        pkg.set_fast_tree(1)
        try:
            sc = pkg.Scene(sd)
        finally:
            pkg.set_fast_tree(-1)
        try:
            for walk in ((True, False) if sc.walk() else (False,)):
                sc.set_walk(walk)
                for anyhit in (False, True):
                    got = sc.debug_soft_lit(rays, hits, pixels, sl, units, samples, seed=seed, level=level, anyhit=anyhit)
                    bad = np.argwhere(got != want)
                    assert len(bad) == 0, f"{name} level {level} walk {walk} anyhit {anyhit}: {len(bad)} counts differ, first {bad[:5].tolist()}"
        finally:
            sc.close()

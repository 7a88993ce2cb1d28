"""Shading fuzz (run on the GPU box): every shading entry against the oracle's recursive per-ray driver.  Each iteration draws a scene
(the kinds of fuzz_render.py, plus meshes with spheres in front of them), random materials, 0-8 point lights and 0-3 spherical lights
(radius 0-0.5, 1-32 samples, unit tables of 1-4096 vectors, random seeds), a depth 0-16 (mostly 0-4), and one mode:
  * frame: cgrt_render_soft (with spherical lights) or cgrt_render (without) against OracleScene.render_soft / render;
  * aa:    cgrt_render_aa against the oracle's 2W x 2H frame, resolved by the plain loop below (include/cgrt.h: the four sub-samples
           summed in the reference's loop order, then divided by 5.0f);
  * rays:  cgrt_shade_rays on tests/rayfam.py families plus random rays about the scene, against OracleScene.shade_rays.
RGB within 1e-5 (NaN at the same positions), ray counts equal by kind; where the scene has a certified walk, the same call in the
quad-per-ray kernel shape and on the exact walk must give the same bytes.
Every iteration also runs an occlusion leg on its scene (its own generator): shadow rays spawned from the oracle's hits towards the
iteration's lights and random ones, plus epsilon-boundary rays (tools/occlfam.py), through cgrt_debug_trace_shadow in every kernel
shape and on every path (n on the host, length on the device with the grid for a larger capacity, paired with a mirror list where
the shape allows it); each verdict `hit && !(t + 0.001f >= dist)` must equal the oracle's.
Usage: python tools/fuzz_shade.py [seconds] [seed]; tests/test_fuzz_gpu.py calls run() over the committed seed list."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as e
import occlfam
import rayfam
pkg = e.load_package(); orc = e.load_oracle()

MODES = ("frame", "aa", "rays")
COUNT_KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays")
THREADS = 16


def resolve_aa(sub, W, H):
    """The reference's antiAliasing branch (main.cpp:663-687) over a 2W x 2H frame, one pixel at a time: color starts at 0, adds the
    sub-samples row by row (yc outer, xc inner), then color / (2.0f * 2.5f)."""
    s = np.asarray(sub, np.float32).reshape(2 * H, 2 * W, 3)
    out = np.zeros((H, W, 3), np.float32)
    div = np.float32(2.0) * np.float32(2.5)
    for y in range(H):
        for x in range(W):
            c = np.zeros(3, np.float32)
            for yc in (2 * y, 2 * y + 1):
                for xc in (2 * x, 2 * x + 1):
                    c = c + s[yc, xc]
            out[y, x] = c / div
    return out.reshape(W * H, 3)


def _scene(rng):
    kind = int(rng.integers(0, 5))
    if kind == 0: sd = pkg.scenes.make_dragon(int(rng.choice([2000, 12000])), seed=int(rng.integers(1, 1 << 30)))
    elif kind == 1: sd = pkg.scenes.make_dragon_irregular(int(rng.choice([4000, 12000])), seed=int(rng.integers(1, 1 << 30)))
    elif kind == 2: sd = pkg.scenes.make_blob(int(rng.choice([300, 3000])), seed=int(rng.integers(1, 1 << 30)))
    else: sd = pkg.scenes.SceneData.load(os.path.join(ROOT, "tests/golden/scenes", str(rng.choice(["cornell", "monkey", "cube"])) + ".npz"))
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3]
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, np.maximum((hi - lo) / 2, np.float32(1e-3))
    spheres = np.zeros((0, 5), np.float32)
    if kind == 4 or rng.integers(0, 4) == 0:  # spheres among and in front of the mesh: hits that keep a mesh's material
        ns = int(rng.integers(1, 4))
        ctr = c + rng.uniform(-1.2, 1.2, (ns, 3)) * ext
        rad = rng.uniform(0.05, 0.4, (ns, 1)) * ext.max()
        spheres = np.concatenate([ctr, rad, -np.ones((ns, 1))], 1).astype(np.float32)
    nm = int(sd.materials.shape[0])
    mats = rng.uniform(0, 1, (nm, 8)).astype(np.float32)
    mats[:, 6] = rng.choice([1.0, 5.0, 20.0, 80.0], nm)  # shininess
    if rng.integers(0, 2): mats[rng.integers(0, nm), 3:6] = 0.0  # a material that reflects nothing
    return kind, pkg.scenes.SceneData(pos_nrm=sd.pos_nrm, tri=sd.tri, tri_mesh=sd.tri_mesh, materials=mats, spheres=spheres), c, ext


def _lights(rng, c, ext):
    nl = int(rng.integers(0, 9))
    lights = np.concatenate([c + rng.uniform(-3.0, 3.0, (nl, 3)) * ext, rng.uniform(0.1, 1.0, (nl, 3))], 1).astype(np.float32)
    ns = int(rng.choice([0, 0, 1, 2, 3]))
    sph = np.concatenate([c + rng.uniform(-2.0, 2.0, (ns, 3)) * ext, rng.uniform(0.0, 0.5, (ns, 1)), rng.uniform(0.2, 1.0, (ns, 3))],
                         1).astype(np.float32)
    if ns and rng.integers(0, 4) == 0: sph[0, 3] = 0.0  # radius 0: every sample at the centre
    soft = {}
    if ns:
        soft = dict(spherical=sph, units=pkg.unit_vector_table(int(rng.choice([1, 2, 7, 64, 1000, 4096])), int(rng.integers(0, 1 << 20))),
                    samples=int(rng.integers(1, 33)), seed=int(rng.integers(0, 1 << 32, dtype=np.uint64)))
    return lights, soft


def _rays(rng, sd, o, c, ext, cam):
    primary = orc.generate_rays(cam, 12, 9)
    fam = rayfam.families(sd, o.nodes()[1], primary, rng=np.random.RandomState(int(rng.integers(0, 1 << 31))), n_random=300)
    pick = [str(k) for k in rng.choice(sorted(fam), min(len(fam), 4), replace=False)]
    n = 400
    o_ = c + rng.uniform(-2.5, 2.5, (n, 3)) * ext
    d = (c + rng.uniform(-0.8, 0.8, (n, 3)) * ext - o_) * rng.uniform(0.05, 5.0, (n, 1))  # non-unit, aimed into the scene
    t = np.where(rng.random(n) < 0.2, rng.uniform(0.0, 4.0, n), rayfam.FMAX)
    rnd = np.concatenate([o_, d, t[:, None]], 1).astype(np.float32)
    rays = np.concatenate([fam[k] for k in pick] + [rnd]).astype(np.float32)
    return np.ascontiguousarray(rays[rng.permutation(len(rays))[:3000]])


def _compare(got, gst, want, wc, stats):
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    m = ~np.isnan(got)
    eq = got[m].view(np.uint32) == want[m].view(np.uint32)  # (equal infinities included)
    with np.errstate(invalid="ignore"):  # (inf - inf of bit-equal entries, dropped by ~eq)
        err = float(np.abs(got[m].astype(np.float64) - want[m])[~eq].max(initial=0.0))
    stats["max_err"] = max(stats["max_err"], err)
    ok = err <= 1e-5
    if any(gst[k] != wc[k] for k in COUNT_KEYS):
        stats["bad_counts"] += 1; ok = False
    return ok


def _occlusion(rng, sc, o, sd, lights, c, ext, cam):
    """The occlusion leg: False when a verdict of any shape / path differs from the oracle's."""
    base = np.concatenate([orc.generate_rays(cam, 16, 12), occlfam.aimed_rays(sd, 200, rng)])
    extra = np.concatenate([lights[:, :3], (c + rng.uniform(-1.5, 1.5, (2, 3)) * ext).astype(np.float32)])
    sr, sdist = occlfam.spawned(o, sd, base, rng, extra_lights=extra, nrandom=0, max_points=200, threads=THREADS)
    br, bd = occlfam.boundary(o, sr, threads=THREADS, max_rays=200, rng=rng)
    rays, dist = np.concatenate([sr, br]), np.concatenate([sdist, bd])
    k = rng.permutation(len(rays))[:int(rng.choice([1, 17, 64, 700, 2000]))]
    k = k[: max(1, len(k) // 2 * 2)] if len(k) > 1 else k
    rays, dist = np.ascontiguousarray(rays[k]), np.ascontiguousarray(dist[k])
    n = len(rays)
    want, ref = occlfam.reference(o, rays, dist, threads=THREADS)
    dmul = 2 if n % 2 == 0 else 1
    ok = True
    for shape in (-1, 0, 1, 2, 3):
        pkg.set_kernel_shape(shape)
        calls = [dict(how=0), dict(how=1, dmul=dmul, capacity=n + int(rng.integers(0, 200)), expected=int(rng.choice([0, 1, n, 50 * n])))]
        if sc.walk() and shape in (-1, 0, 2):
            calls.append(dict(how=2, dmul=dmul, capacity=n + 5, mirror_rays=rays[rng.permutation(n)[: int(rng.integers(0, n + 1))]],
                              mirror_capacity=int(rng.integers(0, 100))))
        for kw in calls:
            got = sc.debug_trace_shadow(rays, dist, **kw)
            h = got[0][:n] if kw["how"] == 2 else got[:n]
            ok &= bool(np.isin(h["hit"], (0, 1)).all() and np.array_equal(occlfam.verdict(h["hit"], h["t"], dist), want))
    pkg.set_kernel_shape(-1)
    return ok


def run(budget=120.0, seed0=1, verbose=True):
    """Fuzz for `budget` seconds from seed `seed0`; returns the statistics (mismatches, bad_counts, walks_differ, shapes_differ must
    be 0)."""
    t_end = time.time() + budget
    stats = dict(iterations=0, frame=0, aa=0, rays=0, spherical=0, spheres=0, deep=0, certified=0, max_err=0.0, mismatches=0,
                 bad_counts=0, walks_differ=0, shapes_differ=0, occlusion=0, bad_verdicts=0)
    t_last = time.time()
    it = 0
    while time.time() < t_end:
        rng = np.random.default_rng([seed0, it, 0x5AADE]); it += 1
        kind, sd, c, ext = _scene(rng)
        lights, soft = _lights(rng, c, ext)
        level = int(rng.choice([0, 1, 2, 3, 4, 2, 3, 4, 1, 2, 6, 9, 16]))
        mode = MODES[int(rng.integers(0, 3))]
        W, H = int(rng.choice([8, 16, 24, 40])), int(rng.choice([6, 12, 20, 30]))
        cam = np.asarray(pkg.scenes.default_camera(W, H), np.float32).copy()
        cam[3:6] = rng.uniform(-3.0, 3.0, 3).astype(np.float32)
        cam[6] = np.float32(rng.uniform(0.6, 4.0))
        sc, o = pkg.Scene(sd), orc.OracleScene(sd)
        if mode == "frame":
            def call():
                return sc.render_soft(cam, W, H, lights=lights, max_level=level, **soft) if soft else sc.render(cam, W, H, lights=lights, max_level=level)
            want, wc = o.render_soft(cam, W, H, lights, max_level=level, threads=THREADS, by_kind=True, **soft)
        elif mode == "aa":
            def call():
                return sc.render_aa(cam, W, H, lights=lights, max_level=level, **soft)
            sub, wc = o.render_soft(cam, 2 * W, 2 * H, lights, max_level=level, threads=THREADS, by_kind=True, **soft)
            want = resolve_aa(sub, W, H)
        else:
            rays = _rays(rng, sd, o, c, ext, cam)
            def call():
                return sc.shade_rays(rays, lights=lights, max_level=level, **soft)
            want, wc = o.shade_rays(rays, lights, max_level=level, threads=THREADS, **soft)
        pkg.set_kernel_shape(0)  # lane per ray
        got, gst = call()
        bad = not _compare(got, gst, want, wc, stats)
        certified = bool(sc.walk())
        if certified:
            stats["certified"] += 1
            pkg.set_kernel_shape(1)  # quad per ray
            gq, _ = call()
            if gq.tobytes() != got.tobytes():
                stats["shapes_differ"] += 1; bad = True
            pkg.set_kernel_shape(-1)
            sc.set_walk(False)
            g0, _ = call()
            if g0.tobytes() != got.tobytes():
                stats["walks_differ"] += 1; bad = True
        pkg.set_kernel_shape(-1)
        if certified:
            sc.set_walk(True)  # (the occlusion leg runs on the scene's default walk)
        if not _occlusion(np.random.default_rng([seed0, it - 1, 0x0CC1]), sc, o, sd, lights, c, ext, cam):
            stats["bad_verdicts"] += 1; bad = True
        stats["occlusion"] += 1
        stats[mode] += 1
        stats["spherical"] += bool(soft)
        stats["spheres"] += len(sd.spheres) > 0
        stats["deep"] += level > 4
        if bad:
            stats["mismatches"] += 1
            print("MISMATCH: seed", seed0, "iteration", it - 1, "mode", mode, "kind", kind, "tris", sd.ntris, "spheres", len(sd.spheres),
                  f"{W}x{H} level {level} lights {len(lights)} spherical {len(soft.get('spherical', ()))}", "counts", gst, wc, flush=True)
        stats["iterations"] += 1
        o.close(); sc.close()
        if verbose and time.time() - t_last > 45:
            t_last = time.time()
            print("progress:", stats, flush=True)
    return stats


if __name__ == "__main__":
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    stats = run(budget, seed0)
    print("shade fuzz:", stats, "seed", seed0, "seconds", budget)
    sys.exit(1 if (stats["mismatches"] or stats["bad_counts"] or stats["walks_differ"] or stats["shapes_differ"]) else 0)

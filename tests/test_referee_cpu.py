"""The CPU oracle against the float64 referee (tests/hp_ref.py): the one place where results are checked against geometry and the
reference's documented behaviour instead of against a twin written in the same arithmetic.  No GPU.  Bounds are derived in
hp_ref's docstring; the rays float32 may decide either way are classed, counted and capped (referee_cases.AMBIGUOUS_CAP), and
`pytest -rA` prints the share per scene and class."""
import numpy as np
import pytest

import hp_ref
import raycam_ref
import rayfam
import referee_cases as cases

U = hp_ref.U
# Measured on the CPU by test_oracle_shading_against_the_referee (largest |dRGB| on stable pixels, by scene); the frame each came
# from is in referee_cases.RGB_MEASURED's comment and DESIGN.md section 3.  The oracle must stay within 1.5 x, the device gets 4 x.
RGB_MEASURED = cases.RGB_MEASURED
RGB_CPU_FACTOR = 1.5


def _oracle_got(res):
    return cases.as_got(res["hit"], res["t"], res["prim"], res["material"], res["normal"])


@pytest.mark.parametrize("name", cases.SMALL + cases.LARGE)
def test_oracle_hits_against_the_referee(pkg, orc, scene_data, name):
    sd = cases.scene(pkg, scene_data, name)
    fam = cases.ray_families(pkg, orc, sd, name)
    rays, spans = cases.concat(fam)
    R = hp_ref.Referee(sd)
    ref = R.nearest_hit(rays)
    clear = cases.check_caps(name, ref, spans)
    assert ref["hit"][clear].any() and (~ref["hit"][clear]).any()
    o = orc.OracleScene(sd)
    bvh, brute = _oracle_got(o.intersect(rays)), _oracle_got(o.intersect(rays, brute_force=True))
    cases.check_hits(f"{name}/oracle brute force", ref, brute, clear)
    cases.check_hits(f"{name}/oracle tree", ref, bvh, clear)
    cases.check_no_false_miss(f"{name}/oracle tree", ref, bvh, spans)
    cases.check_degenerate_flagged(name, R, rays, ref, spans)
    cases.check_f4(name, R, rays, ref, spans)
    deg = cases.in_families(spans, len(rays), cases.DEGENERATE)
    print(f"[referee] {name}: degenerate families {int(deg.sum())} rays, {int((deg & ref['amb']).sum())} flagged; tree verdict differs from the truth on "
          f"{int((bvh['hit'] != ref['hit']).sum())} rays in all, brute force on {int((brute['hit'] != ref['hit']).sum())}")


# -------------------------------------------------------------------------------------------------------------------------------
# the six element-wise primitives, on rayfam.primitive_inputs(): the inputs of the bit-parity tests
# -------------------------------------------------------------------------------------------------------------------------------
def check_primitives(label, inp, f):
    """f: name -> callable with the oracle module's signatures and result layouts (hit, t, normal, pad)."""
    tri, r = inp["triangle"]
    hit, t, nrm, margin, tb, nb = hp_ref.ray_triangle(tri, r)
    got = f["ray_triangle"](tri, r)
    ok = ~margin
    assert 0.3 < ok.mean(), f"{label}: only {ok.mean():.2%} of the triangle rows are clear"
    assert np.array_equal(got["hit"][ok] != 0, hit[ok]), f"{label}: ray-triangle verdict differs on {int(((got['hit'] != 0) != hit)[ok].sum())} clear rows"
    both = ok & hit
    rel = np.abs(got["t"][both].astype(np.float64) - t[both]) / t[both]
    assert np.all(rel <= tb[both]), f"{label}: ray-triangle t outside its bound, worst {np.max(rel / tb[both]):.3g} x"
    ang = hp_ref.angle(got["normal"][both], nrm[both])
    assert np.all(ang <= nb[both]), f"{label}: ray-triangle normal outside its bound, worst {np.max(ang / nb[both]):.3g} x"
    print(f"[referee] {label}: ray_triangle {int(ok.sum())} clear rows ({int(both.sum())} hits), t worst {np.max(rel / tb[both]):.3f} x bound, normal worst {np.max(ang / nb[both]):.3f} x bound")

    D, nn, margin, angb, derr = hp_ref.triangle_plane(inp["tri9"])
    pl = np.asarray(f["triangle_plane"](inp["tri9"]))
    ok = ~margin
    ang = hp_ref.angle(pl[ok, 1:4], nn[ok])
    assert np.all(ang <= angb[ok]) and np.all(np.abs(pl[ok, 0] - D[ok]) <= derr[ok]), f"{label}: triangle_plane outside its bounds"
    print(f"[referee] {label}: triangle_plane {int(ok.sum())} clear rows, normal worst {np.max(ang / angb[ok]):.3f} x bound, D worst {np.max(np.abs(pl[ok, 0] - D[ok]) / derr[ok]):.3f} x bound")

    pl2, pin = rayfam.plane_and_points(inp, pl)
    hit, t, margin, tb = hp_ref.ray_plane(pl2, inp["plane_rays"])
    got = f["ray_plane"](pl2, inp["plane_rays"])
    ok = ~margin
    assert np.array_equal(got["hit"][ok] != 0, hit[ok]), f"{label}: ray-plane verdict differs on {int(((got['hit'] != 0) != hit)[ok].sum())} clear rows"
    both = ok & hit
    rel = np.abs(got["t"][both].astype(np.float64) - t[both]) / t[both]
    assert np.all(rel <= tb[both]), f"{label}: ray-plane t outside its bound, worst {np.max(rel / tb[both]):.3g} x"
    inside, margin = hp_ref.point_in_triangle(pin)
    gp = np.asarray(f["point_in_triangle"](pin)) != 0
    ok2 = ~margin
    assert np.array_equal(gp[ok2], inside[ok2]), f"{label}: point_in_triangle differs on {int((gp != inside)[ok2].sum())} clear rows"
    print(f"[referee] {label}: ray_plane {int(ok.sum())} clear rows, t worst {np.max(rel / tb[both]):.3f} x bound; point_in_triangle {int(ok2.sum())} clear rows, {int(inside[ok2].sum())} inside")

    box, r = inp["box"]
    hit, t, inside, margin = hp_ref.ray_box(box, r)
    got = f["ray_box"](box, r)
    ok = ~margin
    assert 0.5 < ok.mean()
    assert np.array_equal(got["hit"][ok] != 0, hit[ok]), f"{label}: ray-box verdict differs on {int(((got['hit'] != 0) != hit)[ok].sum())} clear rows"
    assert np.array_equal(got["pad"] != 0, inside), f"{label}: starts-inside differs (exact comparisons: every row)"
    both = ok & hit
    rel = np.abs(got["t"][both].astype(np.float64) - t[both]) / np.abs(t[both])
    assert np.all(rel <= hp_ref.K_B * U), f"{label}: ray-box t outside {hp_ref.K_B} * 2^-24, worst {rel.max() / U:.3g} u"
    print(f"[referee] {label}: ray_box {int(ok.sum())} clear rows ({int(both.sum())} hits, {int((inside & ok).sum())} start inside), t worst {rel.max() / U:.3f} u (allowed {hp_ref.K_B})")

    sph, r = inp["sphere"]
    hit, t, nrm, margin, tb, nb = hp_ref.ray_sphere(sph, r)
    got = f["ray_sphere"](sph, r)
    ok = ~margin
    assert 0.5 < ok.mean()
    assert np.array_equal(got["hit"][ok] != 0, hit[ok]), f"{label}: ray-sphere verdict differs on {int(((got['hit'] != 0) != hit)[ok].sum())} clear rows"
    both = ok & hit
    rel = np.abs(got["t"][both].astype(np.float64) - t[both]) / t[both]
    assert np.all(rel <= tb[both]), f"{label}: ray-sphere t outside its bound, worst {np.max(rel / tb[both]):.3g} x"
    ang = hp_ref.angle(got["normal"][both], nrm[both])
    assert np.all(ang <= nb[both]), f"{label}: ray-sphere normal outside its bound, worst {np.max(ang / nb[both]):.3g} x"
    print(f"[referee] {label}: ray_sphere {int(ok.sum())} clear rows ({int(both.sum())} hits), t worst {np.max(rel / tb[both]):.3f} x bound, normal worst {np.max(ang / nb[both]):.3f} x bound")


def test_oracle_primitives_against_the_referee(orc):
    f = {k: getattr(orc, k) for k in ("ray_triangle", "triangle_plane", "ray_plane", "point_in_triangle", "ray_box", "ray_sphere")}
    check_primitives("oracle", rayfam.primitive_inputs(), f)


# -------------------------------------------------------------------------------------------------------------------------------
# cameras
# -------------------------------------------------------------------------------------------------------------------------------
def camera_cases(pkg):
    k = np.float32(0.01745329251994329576923690768489)
    out = [("default 64x48", pkg.scenes.default_camera(64, 48), 64, 48, None)]
    out.append(("rolled, off-centre", np.float32([0.3, -0.2, 0.5, -35 * k, 140 * k, 25 * k, 7.5, 70 * k, 1.6]), 40, 25, None))
    out.append(("rect", np.float32([0, 0, 0, 80 * k, -10 * k, 0, 1.2, 30 * k, 1.0]), 33, 33, (5, 7, 29, 20)))
    return out


def check_camera(label, cam, W, H, rect, rays):
    o, d = hp_ref.camera_rays(cam, W, H, rect)
    rays = np.asarray(rays, np.float32).reshape(-1, 7).astype(np.float64)
    ang = hp_ref.angle(rays[:, 3:6], d)
    scale = abs(float(cam[6])) + float(np.linalg.norm(np.asarray(cam[:3], np.float64)))
    oerr = np.linalg.norm(rays[:, :3] - o, axis=1)
    print(f"[referee] camera {label}: direction worst {ang.max() / U:.2f} u, origin worst {oerr.max() / (U * scale):.2f} u of scale (allowed {hp_ref.K_CAM:g})")
    assert ang.max() <= hp_ref.K_CAM * U, f"{label}: a direction is {ang.max() / U:.1f} * 2^-24 rad from the referee's"
    assert oerr.max() <= hp_ref.K_CAM * U * scale
    assert np.all(np.abs(np.linalg.norm(rays[:, 3:6], axis=1) - 1) <= 8 * U) and np.all(rays[:, 6] == hp_ref.FLT_MAX)


def check_raycam(label, cam, W, H, rays, **region):
    o, d, oerr, aerr = hp_ref.raycam_rays(np.frombuffer(bytes(cam), np.float32), W, H, **region)
    rays = np.asarray(rays, np.float32).reshape(-1, 7).astype(np.float64)
    assert len(rays) == len(o)
    ang = hp_ref.angle(rays[:, 3:6], d)
    od = np.linalg.norm(rays[:, :3] - o, axis=1)
    print(f"[referee] ray camera {label}: direction worst {np.max(ang / aerr):.3f} x bound, origin worst {np.max(od / np.maximum(oerr, 1e-300)):.3f} x bound")
    assert np.all(ang <= aerr) and np.all(od <= oerr), f"{label}: ray camera outside its bounds"


def test_oracle_camera_against_the_referee(pkg, orc):
    for label, cam, W, H, rect in camera_cases(pkg):
        check_camera(label, cam, W, H, rect, orc.generate_rays(cam, W, H, rect))


def raycam_cases(pkg, W=37, H=23):
    cams = dict(raycam_ref.camera_set(pkg, W, H))
    cams["tile"] = raycam_ref.pinhole(pkg, W, H).tile(W, 2 * H)
    cams["far tile"] = raycam_ref.ortho(pkg, W, H).tile(-3000, 4111)
    cams["trackball"] = pkg.RayCamera.from_trackball(pkg.scenes.default_camera(W, H), W, H)
    return cams, W, H


def test_raycam_restatement_against_the_referee(pkg):
    cams, W, H = raycam_cases(pkg)
    for label, cam in cams.items():
        check_raycam(label, cam, W, H, raycam_ref.rays_of(cam, W, H))
    cam = cams["mixed"]
    check_raycam("mixed, region", cam, W, H, raycam_ref.rays_of(cam, W, H, 5, 3, 11, 7), x0=5, y0=3, w=11, h=7)
    # the trackball conversion is the Trackball camera itself, up to the pixel centre convention (corner sampling: no half pixel)
    o, d = hp_ref.camera_rays(pkg.scenes.default_camera(W, H), W, H)
    o2, d2, _, _ = hp_ref.raycam_rays(np.frombuffer(bytes(cams["trackball"]), np.float32), W, H)
    assert hp_ref.angle(d, d2).max() < 8 * U and np.abs(o - o2).max() < 8 * U * 3


# -------------------------------------------------------------------------------------------------------------------------------
# shading
# -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    return cases.Frames()


@pytest.mark.parametrize("frame", sorted(cases.FRAMES))
def test_oracle_shading_against_the_referee(pkg, orc, scene_data, frames, frame):
    sd, cam, rays, L, depth, rgb, unstable, why = frames.frame(pkg, orc, scene_data, frame)
    name = cases.FRAMES[frame][0]
    print(f"[referee] {frame}: unstable rays by class {why}")
    assert rgb.max() > 0.05 or name == "spheres", "the frame is black: nothing is being compared"
    o = orc.OracleScene(sd)
    got, _ = o.shade_rays(rays, L, max_level=depth)
    cases.check_rgb(f"{frame}/oracle shade_rays", rgb, unstable, got, RGB_CPU_FACTOR * RGB_MEASURED[name])
    if cam is not None:
        W = cases.SHADE_W
        frame_rgb, _ = o.render(cam, W, W, L, max_level=depth)
        cases.check_rgb(f"{frame}/oracle render", rgb, unstable, frame_rgb, RGB_CPU_FACTOR * RGB_MEASURED[name])


def test_mirror_threshold_is_classed_unstable(pkg, scene_data):
    """ks.z within 1e-6 of 0.01 (class g): float32's 0.01 is not the real 0.01, so which side of main.cpp:246 such a material falls on is
    not for the referee to decide: every pixel that sees it is unstable, and no other."""
    sd = cases.scene(pkg, scene_data, "mirrorblob")
    sd.materials = sd.materials.copy()
    sd.materials[4, 3:6] = (0.3, 0.3, 0.01)  # the occluder
    rng = np.random.RandomState(3)
    o = np.float64([-1.0, 1.0, -1.0]) + 0.02 * rng.normal(size=(200, 3))
    tgt = np.float64([-0.72, 0.72, -0.72]) + 0.6 * rng.uniform(-1, 1, (200, 3))
    rays = np.concatenate([o, tgt - o, np.full((200, 1), hp_ref.FLT_MAX)], 1).astype(np.float32)
    R = hp_ref.Referee(sd)
    h = R.nearest_hit(rays)
    _, unstable, _ = R.shade(rays, sd.point_lights, 1)
    on = h["hit"] & (h["material"] == 4)
    assert 20 < on.sum() < 180
    assert unstable[on].all() and unstable[~on].mean() < 0.1


# -------------------------------------------------------------------------------------------------------------------------------
# visibility
# -------------------------------------------------------------------------------------------------------------------------------
def visibility_cases(pkg, scene_data, name, n=3000, seed=17):
    """Segments (rays with a finite t) between random points about the scene, and surface points with the scene's lights."""
    sd = cases.scene(pkg, scene_data, name)
    rng = np.random.RandomState(seed)
    p = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    c, ext = (lo + hi) / 2, (hi - lo) / 2
    a = c + rng.uniform(-1.4, 1.4, (n, 3)) * ext
    b = c + rng.uniform(-1.4, 1.4, (n, 3)) * ext
    d = b - a
    seg = np.concatenate([a, d, np.ones((n, 1))], 1)  # unnormalised direction, t = 1: the segment a .. b
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    seg[n // 2:, 3:6] /= ln[n // 2:]
    seg[n // 2:, 6] = ln[n // 2:, 0] * rng.uniform(0.3, 1.0, n - n // 2)
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    k = tri[rng.randint(0, len(tri), n)]
    w = rng.dirichlet((2, 2, 2), n)
    pts = (p[k] * w[:, :, None]).sum(1)
    return sd, seg.astype(np.float32), pts.astype(np.float32)


def shadow_truth(R, pts, light):
    """pointInShadow of float32 points for one light: hp_ref's own rule and band, the ones its shading uses."""
    shadow, amb, _ = R.point_in_shadow(np.asarray(pts, np.float32).astype(np.float64), light)
    return shadow, amb


@pytest.mark.parametrize("name", ["cornell", "monkey", "mirrorblob"])
def test_oracle_visibility_against_the_referee(pkg, orc, scene_data, name):
    sd, seg, pts = visibility_cases(pkg, scene_data, name)
    R = hp_ref.Referee(sd)
    o = orc.OracleScene(sd)
    occ, amb = R.any_hit(seg)
    got = o.intersect(seg)["hit"] != 0
    assert amb.mean() <= cases.AMBIGUOUS_CAP and 0.05 < occ.mean() < 0.95
    bad = (got != occ) & ~amb
    assert not bad.any(), f"{name}: occlusion differs on {int(bad.sum())} clear segments, first {np.nonzero(bad)[0][:5]}"
    for li, light in enumerate(cases.frame_lights(sd, None)):
        want, amb = shadow_truth(R, pts, light)
        # the oracle's verdict as main.cpp:104-135 drives its closest hit, in float32
        to = (light[:3] - pts).astype(np.float32)
        ln = np.sqrt((to * to).sum(1, dtype=np.float32), dtype=np.float32)
        dirn = (to / ln[:, None]).astype(np.float32)
        org = (pts + np.float32(0.001) * dirn).astype(np.float32)
        res = o.intersect(np.concatenate([org, dirn, np.full((len(pts), 1), hp_ref.FLT_MAX, np.float32)], 1))
        got = (res["hit"] != 0) & ~((res["t"] + np.float32(0.001)).astype(np.float32) >= ln)
        share = float(amb.mean())
        print(f"[referee] {name}: light {li}: {int(want.sum())} of {len(pts)} surface points in shadow, ambiguous {share:.3%}; occlusion ambiguous as above")
        assert share <= cases.AMBIGUOUS_CAP, f"{name}: {share:.2%} of the shadow verdicts are ambiguous"
        bad = (got != want) & ~amb
        assert not bad.any(), f"{name}: shadow verdict differs on {int(bad.sum())} clear points, first {np.nonzero(bad)[0][:5]}"

"""The device entries against the float64 referee (tests/hp_ref.py): the assertions, bounds, caps and exclusions of
tests/test_referee_cpu.py with the HIP kernels in the oracle's place.  The referee's answers are computed on the host and cached per
scene; the set of ambiguous rays depends on scene and rays only, so the device is excused on exactly the rays the oracle was."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")  # before the package opens the HIP runtime, as in the other tensor tests

import hp_ref  # noqa: E402
import rayfam  # noqa: E402
import referee_cases as cases  # noqa: E402
import test_referee_cpu as cpu  # noqa: E402

pytestmark = pytest.mark.gpu
U = hp_ref.U
# Largest |dRGB| of the CPU oracle against the referee on stable pixels, by scene (measured on the CPU only: referee_cases.RGB_MEASURED
# names the frames); the device is allowed RGB_DEVICE_FACTOR = 4 times that.
RGB_MEASURED = cases.RGB_MEASURED
RGB_DEVICE_FACTOR = cases.RGB_DEVICE_FACTOR



@pytest.fixture(scope="module")
def frames():
    return cases.Frames()


@pytest.fixture(scope="module")
def geometry():
    return {}


def _rays(pkg, r7):
    return np.ascontiguousarray(r7, np.float32).view(pkg.RAY_DTYPE).reshape(-1)


def _device_got(hits, normals):
    return cases.as_got(hits["hit"], hits["t"], hits["prim_id"], hits["material_id"], normals)


def _scene_case(_geometry, pkg, orc, scene_data, name):
    if name not in _geometry:
        sd = cases.scene(pkg, scene_data, name)
        rays, spans = cases.concat(cases.ray_families(pkg, orc, sd, name))
        _geometry[name] = (sd, rays, spans, hp_ref.Referee(sd).nearest_hit(rays))
    return _geometry[name]


@pytest.mark.parametrize("name", cases.SMALL + cases.LARGE)
def test_device_hits_against_the_referee(pkg, orc, scene_data, geometry, name):
    sd, rays, spans, ref = _scene_case(geometry, pkg, orc, scene_data, name)
    clear = cases.check_caps(name, ref, spans)
    pkg.set_fast_tree(1)  # the certified walk wherever a fast tree can be built
    try:
        sc = pkg.Scene(sd)
    finally:
        pkg.set_fast_tree(-1)
    r = _rays(pkg, rays)
    fast = sc.build_info()["fast_tree"]
    try:
        for certified in ((True, False) if fast else (False,)):
            if fast:
                sc.set_walk(certified)
            for shape in (-1, 0, 1, 2, 3):
                pkg.set_kernel_shape(shape)
                label = f"{name}/device {'certified' if certified else 'exact'} walk, shape {shape}"
                got = _device_got(*sc.intersect(r))
                cases.check_hits(label, ref, got, clear)
                cases.check_no_false_miss(label, ref, got, spans)
        pkg.set_kernel_shape(-1)
        cases.check_hits(f"{name}/device brute force", ref, _device_got(*sc.intersect_brute(r)), clear)
    finally:
        pkg.set_kernel_shape(-1)
        sc.close()


def _device_primitives(pkg):
    def hit_t_n(fn):
        def call(a, rays):
            t, hit, nrm = fn(a, _rays(pkg, rays))
            return dict(hit=hit, t=t, normal=nrm)
        return call

    def plane(a, rays):
        t, hit = pkg.ray_plane(a, _rays(pkg, rays))
        return dict(hit=hit, t=t)

    def box(a, rays):
        t, hit, inside = pkg.ray_box(a, _rays(pkg, rays))
        return dict(hit=hit, t=t, pad=inside)

    return dict(ray_triangle=hit_t_n(pkg.ray_triangle), ray_sphere=hit_t_n(pkg.ray_sphere), ray_plane=plane, ray_box=box,
                triangle_plane=pkg.triangle_plane, point_in_triangle=pkg.point_in_triangle)


def test_device_primitives_against_the_referee(pkg):
    cpu.check_primitives("device", rayfam.primitive_inputs(), _device_primitives(pkg))


def test_device_cameras_against_the_referee(pkg, scene_data):
    sc = pkg.Scene(scene_data("cube"))
    for label, cam, W, H, rect in cpu.camera_cases(pkg):
        cpu.check_camera(f"device, {label}", cam, W, H, rect, sc.generate_rays(cam, W, H, rect).view(np.float32).reshape(-1, 7))
    cams, W, H = cpu.raycam_cases(pkg)
    for label, cam in cams.items():
        cpu.check_raycam(f"device, {label}", cam, W, H, sc.generate_rays_raycam(cam, W, H).view(np.float32).reshape(-1, 7))
    sc.close()


@pytest.mark.parametrize("name", ["cornell", "monkey", "mirrorblob"])
def test_device_visibility_against_the_referee(pkg, scene_data, name):
    sd, seg, pts = cpu.visibility_cases(pkg, scene_data, name)
    R = hp_ref.Referee(sd)
    sc = pkg.Scene(sd)
    occ, amb = R.any_hit(seg)
    assert amb.mean() <= cases.AMBIGUOUS_CAP and 0.05 < occ.mean() < 0.95
    got = sc.occluded(_rays(pkg, seg))
    bad = (got != occ) & ~amb
    assert not bad.any(), f"{name}: occluded differs on {int(bad.sum())} clear segments, first {np.nonzero(bad)[0][:5]}"
    lights = cases.frame_lights(sd, None)
    shadow = sc.in_shadow(pts, lights)
    for li, light in enumerate(lights):
        want, amb = cpu.shadow_truth(R, pts, light)
        assert amb.mean() <= cases.AMBIGUOUS_CAP, f"{name}: {amb.mean():.2%} of the shadow verdicts are ambiguous"
        bad = (shadow[:, li] != want) & ~amb
        assert not bad.any(), f"{name}: in_shadow differs on {int(bad.sum())} clear points for light {li}, first {np.nonzero(bad)[0][:5]}"
    sc.close()


# -------------------------------------------------------------------------------------------------------------------------------
# frames
# -------------------------------------------------------------------------------------------------------------------------------
def _bound(name):
    return RGB_DEVICE_FACTOR * RGB_MEASURED[name]


@pytest.mark.parametrize("frame", sorted(cases.FRAMES))
def test_device_shading_against_the_referee(pkg, orc, scene_data, frames, frame):
    sd, cam, rays, L, depth, rgb, unstable, _ = frames.frame(pkg, orc, scene_data, frame)
    name = cases.FRAMES[frame][0]
    W = cases.SHADE_W
    sc = pkg.Scene(sd)
    try:
        got, _ = sc.shade_rays(_rays(pkg, rays), lights=L, max_level=depth)
        cases.check_rgb(f"{frame}/device shade_rays", rgb, unstable, got, _bound(name))
        if cam is not None:
            got, _ = sc.render(cam, W, W, lights=L, max_level=depth)
            cases.check_rgb(f"{frame}/device render", rgb, unstable, got, _bound(name))
    finally:
        sc.close()


def test_device_primary_frames_and_geometry_buffers(pkg, orc, scene_data, frames):
    """trace_primary (one wave per tile, and the persistent variant) and the planes of render_aov_tensor against the referee's hit record of
    the frame's own rays: depth = t, position = o + t d, normal, albedo = kd, ids, mask."""
    W = cases.SHADE_W
    for frame in ("cornell_d2", "monkey_d2", "mixed_d2", "mirrorblob_d3", "spheres_d2"):
        sd, cam, rays, L, depth, _, _, _ = frames.frame(pkg, orc, scene_data, frame)
        ref = hp_ref.Referee(sd).nearest_hit(rays)
        clear = ~ref["amb"]
        assert ref["amb"].mean() <= cases.AMBIGUOUS_CAP
        sc = pkg.Scene(sd)
        assert np.array_equal(sc.generate_rays(cam, W, W).view(np.float32).reshape(-1, 7).view(np.uint32), rays.view(np.uint32)), "the frame's rays are not the referee's input"
        try:
            for mode in (0, 1):
                pkg.set_primary_mode(mode)
                cases.check_hits(f"{frame}/trace_primary mode {mode}", ref, _device_got(*sc.trace_primary(cam, W, W, want_normals=True)), clear)
        finally:
            pkg.set_primary_mode(0)
        out, _, planes = sc.render_aov_tensor(cam, W, W, lights=L, max_level=depth)
        torch.cuda.synchronize()
        P = {k: v.cpu().numpy() for k, v in planes.items()}
        got = cases.as_got(P["mask"].reshape(-1), P["depth"].reshape(-1), P["prim_id"].reshape(-1).view(np.uint32), P["material_id"].reshape(-1),
                           P["normal"].reshape(-1, 3))
        cases.check_hits(f"{frame}/geometry buffers", ref, got, clear)
        both = clear & ref["hit"]
        r64 = rays.astype(np.float64)
        want = r64[:, :3] + r64[:, 3:6] * np.where(ref["hit"], ref["t"], 0.0)[:, None]
        dl = np.linalg.norm(r64[:, 3:6], axis=1)
        K = np.where(ref["sphere"], hp_ref.K_S, hp_ref.K_T)
        tol = K * U * ref["cond"] * ref["t"] * dl + 4 * U * (np.linalg.norm(r64[:, :3], axis=1) + dl * ref["t"])
        err = np.linalg.norm(P["position"].reshape(-1, 3) - want, axis=1)
        assert np.all(err[both] <= tol[both]), f"{frame}: position plane outside its bound, worst {np.max(err[both] / tol[both]):.3g} x"
        kd = np.zeros((len(rays), 3), np.float32)  # material -1 (a miss, a sphere-only hit): the default Material's kd, read as 0
        has = ref["material"] >= 0
        kd[has] = np.asarray(sd.materials, np.float32).reshape(-1, 8)[ref["material"][has], :3]
        assert np.array_equal(P["albedo"].reshape(-1, 3)[both], kd[both]), f"{frame}: albedo plane is not kd of the hit's material"
        sc.close()


def _second_camera(pkg, W):
    k = np.float32(0.01745329251994329576923690768489)
    return np.float32([0.05, -0.05, 0.0, -15 * k, 205 * k, 0, 3.4, 40 * k, 1.0])


def test_device_batched_frames_against_the_referee(pkg, orc, scene_data, frames):
    """render_views_tensor (two views), a light-set batch and a ray-camera frame, each against the referee's frame of the same rays."""
    W = cases.SHADE_W
    # two views of the mirror blob, depth 3
    sd, cam, rays, L, depth, rgb, unstable, _ = frames.frame(pkg, orc, scene_data, "mirrorblob_d3")
    cam2 = _second_camera(pkg, W)
    rays2 = orc.generate_rays(cam2, W, W)
    _, _, _, _, _, rgb2, unstable2, _ = frames.extra("mirrorblob_d3/view 2", pkg, scene_data, "mirrorblob", rays2, cam2, None, depth)
    assert rgb2.max() > 0.05
    sc = pkg.Scene(sd)
    out, _ = sc.render_views_tensor(np.stack([cam, cam2]), W, W, lights=L, max_level=depth)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(2, -1, 3)
    cases.check_rgb("mirrorblob_d3/render_views_tensor view 0", rgb, unstable, got[0], _bound("mirrorblob"))
    cases.check_rgb("mirrorblob_d3/render_views_tensor view 1", rgb2, unstable2, got[1], _bound("mirrorblob"))
    sc.close()
    # one camera under two light setups: Cornell, depth 2
    sd, cam, rays, L1, depth, rgb1, uns1, _ = frames.frame(pkg, orc, scene_data, "cornell_d2")
    _, _, _, L3, _, rgb3, uns3, _ = frames.frame(pkg, orc, scene_data, "cornell_3l_d2")
    sc = pkg.Scene(sd)
    got, _ = sc.render_light_sets(cam, W, W, [L1, L3], max_level=depth)
    cases.check_rgb("cornell_d2/render_light_sets set 0", rgb1, uns1, got[0], _bound("cornell"))
    cases.check_rgb("cornell_3l_d2/render_light_sets set 1", rgb3, uns3, got[1], _bound("cornell"))
    sc.close()
    # a ray-camera frame of the monkey: the rays are the device's own (held against the referee's camera by the camera test)
    sd = cases.scene(pkg, scene_data, "monkey")
    sc = pkg.Scene(sd)
    rc = pkg.RayCamera.from_trackball(pkg.scenes.default_camera(W, W), W, W)
    rr = sc.generate_rays_raycam(rc, W, W).view(np.float32).reshape(-1, 7)
    _, _, _, L, _, rgbr, unsr, _ = frames.extra("monkey_d2/ray camera", pkg, scene_data, "monkey", rr, None, None, 2)
    out, _ = sc.render_raycams_tensor(rc, W, W, lights=L, max_level=2)
    torch.cuda.synchronize()
    cases.check_rgb("monkey_d2/render_raycams_tensor", rgbr, unsr, out.cpu().numpy().reshape(-1, 3), _bound("monkey"))
    sc.close()

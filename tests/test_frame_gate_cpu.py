"""CPU test of the frame gate's rectangle (capi.cpp frame_gate_rect, include/cgrt.h cgrt_debug_frame_gate) on host-only
scenes: for every camera of the set below and EVERY pixel outside the rectangle the library reports, the per-pixel root gate
(walk_exact.h walk_begin: starts_in_box || ray_box, in float) says "miss" -- evaluated by the oracle's own primitives on the oracle's
own rays (oracle_generate_rays, oracle_ray_box: its ray-box restatement and its strict inside test).  A camera without a rectangle
counts only where the design says there is none: the origin on a box plane or inside the box, a box that reaches behind the camera
plane, a scene with spheres or without meshes.  Cameras that must yield one are asserted to."""
import numpy as np
import pytest

F32 = np.float32
SIZES = [(200, 120), (97, 61), (64, 48)]  # 97 x 61: no multiple of 8; 64 x 48: even, so the axis views have a centre pixel
MESH_SCENES = ["dragon20k", "monkey", "cornell", "dodge"]


@pytest.fixture(scope="module")
def worlds(pkg, orc, scene_data):
    cache = {}

    def get(name):
        if name not in cache:
            sd = pkg.scenes.make_dragon(20_000) if name == "dragon20k" else scene_data(name)
            sc = pkg.Scene(sd, device=-1)
            box = None
            if len(sd.tri):
                box = orc.OracleScene(sd).nodes()[1][0].copy()  # the reference tree's root box ...
                used = np.asarray(sd.pos_nrm, F32).reshape(-1, 6)[np.unique(np.asarray(sd.tri).reshape(-1)), :3]
                assert np.array_equal(box, np.concatenate([used.min(0), used.max(0)])), "... is the exact bound of the mesh vertices"
            cache[name] = (sd, sc, box)
        return cache[name]

    return get


def cam9(look_at, euler, distance, fovy_deg, W, H):
    return np.asarray([*look_at, *euler, distance, np.deg2rad(fovy_deg), F32(W) / F32(H)], F32)


def cameras(pkg, box, W, H, seed):
    """(label, camera, expectation): "rect" = a rectangle must come back, "none" = a listed degenerate case, none may."""
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    c, ext = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    out = [("default", pkg.scenes.default_camera(W, H), "rect")]
    out.append(("near", cam9(c, (0.3, 0.4, 0.0), 0.75 * ext, 50, W, H), "rect"))
    out.append(("far", cam9(c, (0.35, -0.6, 0.1), 40 * ext, 50, W, H), "rect"))
    out.append(("sub-pixel", cam9(c, (0.2, 0.3, 0.0), 4000 * ext, 50, W, H), "rect"))
    # off axis: the box near a corner of the frame, partly outside it, wholly outside it
    out.append(("off-axis corner", cam9(c + [0.9 * ext, 0.5 * ext, 0], (0.1, 0.2, 0.0), 3 * ext, 50, W, H), "rect"))
    out.append(("off-axis cut", cam9(c + [0.0, 1.2 * ext, 0.3 * ext], (-0.4, 2.5, 0.3), 2.5 * ext, 35, W, H), "rect"))
    out.append(("off-axis out of frame", cam9(c + [8 * ext, 0, 0], (0.0, 0.0, 0.0), 4 * ext, 30, W, H), "rect"))
    out.append(("wide", cam9(c, (1.0, 2.0, 3.0), 1.5 * ext, 120, W, H), "rect"))
    # axis-aligned: euler 0 looks along +z exactly (identity quaternion); the centre pixel of an even frame is d = (0, 0, 1)
    out.append(("axis +z", cam9(c.astype(F32), (0, 0, 0), 2 * ext, 50, W, H), "rect"))
    out.append(("axis +z, look_at 0", cam9((0, 0, 0), (0, 0, 0), 3 * ext + float(np.abs(box).max()), 50, W, H), "rect"))
    out.append(("axis -z", cam9(c, (0, np.pi, 0), 2 * ext, 50, W, H), "rect"))
    out.append(("axis x", cam9(c, (0, np.pi / 2, 0), 2 * ext, 50, W, H), "rect"))
    out.append(("axis y", cam9(c, (np.pi / 2, 0, 0), 2 * ext, 50, W, H), "rect"))
    # the origin exactly on the plane x = lo.x, the box ahead: the centre column has d.x = 0 and the gate's x quotient is 0/0
    on = cam9((box[0], c[1], c[2]), (0, 0, 0), 2 * ext, 50, W, H)
    out.append(("origin on a box plane", on, "none"))
    out.append(("origin on a box plane, beside the box", cam9((box[3], hi[1] + ext, c[2]), (0, 0, 0), 2 * ext, 50, W, H), "none"))
    out.append(("origin inside", cam9(c, (0.3, 0.2, 0.0), 0.01 * ext, 50, W, H), "none"))
    out.append(("box partly behind", cam9((hi[0] + 0.05 * ext, c[1], c[2]), (0, 0, 0), 0.0, 50, W, H), "none"))
    out.append(("box partly behind, turned", cam9(c, (0.5, 0.7, 0.0), 0.45 * ext, 50, W, H), "none"))
    rng = np.random.default_rng(seed)
    for k in range(6):
        la = c + rng.uniform(-0.6, 0.6, 3) * ext
        out.append((f"random {k}", cam9(la, rng.uniform(-np.pi, np.pi, 3), rng.uniform(1.7, 6.0) * ext, rng.uniform(20, 100), W, H), "rect"))
    return out


def gate_misses(orc, box, cam, W, H):
    """Per pixel: the root gate's verdict is "miss" (neither the strict inside test nor the reference's ray-box test passes)."""
    rays = orc.generate_rays(cam, W, H)
    v = orc.ray_box(np.broadcast_to(box, (len(rays), 6)), rays)
    return ((v["hit"] == 0) & (v["pad"] == 0.0)).reshape(H, W)


@pytest.mark.parametrize("name", MESH_SCENES)
def test_every_pixel_outside_the_rectangle_misses_the_root_gate(pkg, orc, worlds, name):
    sd, sc, box = worlds(name)
    seen = {"rect": 0, "none": 0}
    tight = 0
    for si, (W, H) in enumerate(SIZES):
        for label, cam, expect in cameras(pkg, box, W, H, seed=1000 + si):
            r = sc.frame_gate(cam, W, H)
            what = f"{name} {W}x{H} {label}"
            if expect == "rect":
                assert r is not None, f"{what}: no rectangle for a camera that must have one"
            else:
                assert r is None, f"{what}: a rectangle {r} for a degenerate camera"
                seen["none"] += 1
                continue
            seen["rect"] += 1
            x0, y0, x1, y1 = r
            assert 0 <= x0 <= x1 <= W and 0 <= y0 <= y1 <= H, f"{what}: {r} leaves the frame"
            miss = gate_misses(orc, box, cam, W, H)
            outside = np.ones((H, W), bool)
            outside[y0:y1, x0:x1] = False
            bad = outside & ~miss
            assert not bad.any(), f"{what}: {int(bad.sum())} pixels outside {r} pass the root gate, first (y, x) = {np.argwhere(bad)[0]}"
            # the rectangle is a bound, not the frame: where the box's outline lies wholly inside the frame (its extreme corners then
            # project into it), the rectangle is the passing pixels' bounding box plus the margin (1 px + a relative term: < 2 px)
            ys, xs = np.nonzero(~miss)
            if len(xs) and xs.min() > 0 and ys.min() > 0 and xs.max() < W - 1 and ys.max() < H - 1:
                assert x0 >= xs.min() - 3 and x1 <= xs.max() + 4 and y0 >= ys.min() - 3 and y1 <= ys.max() + 4, \
                    f"{what}: {r} is loose around x {xs.min()}..{xs.max()}, y {ys.min()}..{ys.max()}"
                tight += 1
    assert seen["rect"] == 3 * 19 and seen["none"] == 3 * 5 and tight >= 3 * 5


def test_the_cameras_that_matter_are_gated(pkg, worlds):
    """The default camera's rectangle on the smoke scene is a proper part of the frame (the gate has something to skip)."""
    sd, sc, box = worlds("dragon20k")
    for W, H in [(1920, 1080), (200, 120), (97, 61)]:
        r = sc.frame_gate(pkg.scenes.default_camera(W, H), W, H)
        assert r is not None
        assert (r[2] - r[0]) * (r[3] - r[1]) < 0.6 * W * H, f"{W}x{H}: {r}"
    assert sc.frame_gate(cam9((50.0, 0, 0), (0, 0, 0), 3.0, 30, 64, 48), 64, 48) == (0, 0, 0, 0), "a box out of the frame: every pixel misses"


def test_no_rectangle_without_a_mesh_gate(pkg, worlds):
    """Spheres are tested for rays that failed the mesh root gate, and a scene without meshes has no gate: never a rectangle."""
    sd, sc, _ = worlds("spheres")
    for W, H in SIZES:
        assert sc.frame_gate(pkg.scenes.default_camera(W, H), W, H) is None
        assert sc.frame_gate(cam9((0, 0, 6), (0.1, 0.2, 0), 30.0, 50, W, H), W, H) is None


def test_non_finite_and_out_of_envelope_cameras_have_no_rectangle(pkg, worlds):
    sd, sc, box = worlds("monkey")
    W, H = 64, 48
    base = pkg.scenes.default_camera(W, H)
    assert sc.frame_gate(base, W, H) is not None
    for k, v in [(0, np.nan), (1, np.inf), (6, np.inf), (6, 1e30), (3, np.nan), (7, 0.0), (7, np.pi), (8, 0.0), (8, -1.0), (8, 1e30), (8, 1e13), (8, 1e-13), (7, 1e-12)]:
        cam = base.copy()
        cam[k] = v
        assert sc.frame_gate(cam, W, H) is None, f"camera field {k} = {v}"


def test_switch_and_arguments(pkg, worlds):
    sd, sc, _ = worlds("monkey")
    L = pkg.lib()
    assert L.cgrt_set_frame_gate(2) != 0 and L.cgrt_set_frame_gate(-1) != 0
    cam = pkg.scenes.default_camera(64, 48)
    r = sc.frame_gate(cam, 64, 48)
    pkg.set_frame_gate(False)
    try:
        assert sc.frame_gate(cam, 64, 48) == r, "the debug entry reports the geometry, not the switch"
    finally:
        pkg.set_frame_gate(True)
    with pytest.raises(pkg.CgrtError):
        sc.frame_gate(cam, 0, 48)
    assert "cgrt_set_frame_gate" in pkg.EXPORTS and "cgrt_debug_frame_gate" in pkg.EXPORTS

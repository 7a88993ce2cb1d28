"""GPU tests of the anti-aliased frame (cgrt_render_aa*, the reference's antiAliasing branch, src/main.cpp:663-687).

With point lights an AA frame is fully determined (include/cgrt.h findings AA1-AA4): it is the library's own 2W x 2H frame, resolved
by summing each pixel's four sub-samples in the reference's loop order onto zero and dividing by 5.0f.  So the device's AA frame
must equal that resolve, done here in numpy float32, BIT FOR BIT; against the oracle it must hold the RGB parity bar (1e-5)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXACT, PREDICTED = 0, 1
TOL = 1e-5  # the RGB parity bar
RAD = np.float32(0.01745329251994329576923690768489)


def _scene(pkg, scene_data, name):
    return pkg.Scene(scene_data(name), device=0)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _resolved_double_frame(pkg, sc, cam, W, H, max_level, **soft):
    """The library's own 2W x 2H frame (cgrt_render / cgrt_render_soft) resolved in numpy float32 in the reference's order."""
    if soft:
        sub, _ = sc.render_soft(cam, 2 * W, 2 * H, max_level=max_level, **soft)
    else:
        sub, _ = sc.render(cam, 2 * W, 2 * H, max_level=max_level)
    return pkg.resolve_aa(sub, W, H)


@pytest.mark.parametrize(
    "name,W,H,depth",
    [("cube", 64, 48, 2), ("monkey", 80, 64, 2), ("spheres", 72, 40, 2), ("cornell", 96, 64, 2), ("cornell", 96, 64, 4),
     ("cornell", 97, 61, 2), ("monkey", 1, 1, 2), ("cornell", 3, 1, 4), ("cornell", 800, 800, 2)],
)
def test_aa_equals_resolved_double_frame_bit_for_bit(pkg, scene_data, name, W, H, depth):
    sc = _scene(pkg, scene_data, name)
    cam = pkg.scenes.default_camera(W, H)
    if name == "spheres":  # (as tests/test_host_mirror.py: the spheres sit around z = 6; they have no material upstream, so they shade black)
        cam = np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
    want = _resolved_double_frame(pkg, sc, cam, W, H, depth)
    got, st = sc.render_aa(cam, W, H, max_level=depth)
    assert got.shape == (W * H, 3)
    assert _same_bits(got, want)
    assert st["primary_rays"] == 4 * W * H
    got_m, st_m = sc.render_aa(cam, W, H, max_level=depth, mapped=True)
    assert _same_bits(got_m, want) and st_m["primary_rays"] == 4 * W * H
    if W * H >= 64:
        assert st["shadow_rays"] > 0  # the primary rays hit the scene
        assert name == "spheres" or (got.sum(1) > 0).mean() > 0.02  # and the frame shows it


def test_aa_of_a_camera_facing_away_is_black(pkg, scene_data):
    sc = _scene(pkg, scene_data, "cornell")
    W, H = 40, 24
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[0:6] = [50.0, 0.0, 0.0, 0.0, 0.0, 0.0]  # looking along +z from (50, 0, -3): nothing in view
    sc.render_aa(pkg.scenes.default_camera(W, H), W, H)  # a frame with hits first: the workspace holds colour
    got, st = sc.render_aa(cam, W, H)
    assert _same_bits(got, _resolved_double_frame(pkg, sc, cam, W, H, 2))
    assert not got.any() and st["primary_rays"] == 4 * W * H and st["shadow_rays"] == 0 and st["levels"] == 0


def test_predicted_frame_without_hits_is_black(pkg, scene_data):
    """A frame of the previous frame's shape takes the predicted path even when none of its rays hits (the AA test above found that
    this case read the first entry of an empty level list): plain frames too."""
    sc = _scene(pkg, scene_data, "cornell")
    W, H = 40, 24
    sc.render(pkg.scenes.default_camera(W, H), W, H)
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[0:6] = [50.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    got, st = sc.render(cam, W, H)
    assert sc.last_render_path() == PREDICTED
    assert not got.any() and st["primary_rays"] == W * H and st["shadow_rays"] == 0 and st["levels"] == 0


def test_aa_depth_zero_is_black(pkg, scene_data):
    sc = _scene(pkg, scene_data, "cornell")
    got, st = sc.render_aa(pkg.scenes.default_camera(16, 8), 16, 8, max_level=0)
    assert not got.any() and st["levels"] == 0


@pytest.mark.parametrize("name,W,H,depth,band", [("cornell", 1920, 1080, 4, (1000, 1128)), ("monkey", 800, 800, 2, None)])
def test_aa_matches_oracle(pkg, orc, scene_data, name, W, H, depth, band):
    """The oracle's 2W x 2H frame (rows y0..y1 of it for the 1080p frame), resolved in numpy, within the RGB parity bar."""
    sd = scene_data(name)
    sc = pkg.Scene(sd, device=0)
    cam = pkg.scenes.default_camera(W, H)
    got, st = sc.render_aa(cam, W, H, max_level=depth)
    assert st["primary_rays"] == 4 * W * H
    y0, y1 = band if band else (0, 2 * H)
    sub, _ = orc.OracleScene(sd).render(cam, 2 * W, 2 * H, sd.point_lights, max_level=depth, y0=y0, y1=y1)
    hb = (y1 - y0) // 2
    ref = pkg.resolve_aa(sub, W, hb)
    mine = got.reshape(H, W, 3)[y0 // 2:y0 // 2 + hb].reshape(-1, 3)
    assert np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max() <= TOL
    assert (ref.sum(1) > 0).mean() > 0.05


def _soft_args(pkg, samples=16, seed=11):
    return dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(4096, 3), samples=samples, seed=seed)


def test_soft_aa_equals_resolved_double_soft_frame(pkg, scene_data):
    """Sub-sample (xc, yc) hashes as pixel yc * 2W + xc: the soft AA frame is the 2W x 2H soft frame of the same table and seed."""
    sc = _scene(pkg, scene_data, "cornell")
    W, H = 61, 37
    cam = pkg.scenes.default_camera(W, H)
    soft = _soft_args(pkg)
    want = _resolved_double_frame(pkg, sc, cam, W, H, 2, **soft)
    got, st = sc.render_aa(cam, W, H, **soft)
    assert _same_bits(got, want)
    assert st["soft_shadow_rays"] > 0 and st["primary_rays"] == 4 * W * H


def test_soft_aa_matches_oracle(pkg, orc, scene_data):
    sd = scene_data("cornell")
    sc = pkg.Scene(sd, device=0)
    W, H = 48, 32
    cam = pkg.scenes.default_camera(W, H)
    soft = _soft_args(pkg, samples=24, seed=5)
    got, _ = sc.render_aa(cam, W, H, **soft)
    sub, _ = orc.OracleScene(sd).render_soft(cam, 2 * W, 2 * H, sd.point_lights, soft["spherical"], soft["units"], samples=soft["samples"],
                                             seed=soft["seed"], max_level=2)
    ref = pkg.resolve_aa(sub, W, H)
    assert np.abs(got.astype(np.float64) - ref.astype(np.float64)).max() <= TOL
    assert (ref.sum(1) > 0).mean() > 0.05


def test_repeated_aa_frames_take_the_predicted_path(pkg, scene_data):
    sc = _scene(pkg, scene_data, "cornell")
    W, H = 160, 96
    cam = pkg.scenes.default_camera(W, H)
    a, sa = sc.render_aa(cam, W, H)
    assert sc.last_render_path() == EXACT
    b, sb = sc.render_aa(cam, W, H)
    assert sc.last_render_path() == PREDICTED
    assert a.tobytes() == b.tobytes()
    keys = ("primary_rays", "shadow_rays", "reflection_rays", "levels")
    assert all(sa[k] == sb[k] for k in keys)
    # after a camera move: still the predicted path (or redrawn), and the exact frame's bytes
    moved = cam.copy()
    moved[4] = np.float32(23.0) * RAD
    c, _ = sc.render_aa(moved, W, H)
    assert sc.last_render_path() in (PREDICTED, 2)
    pkg.set_render_prediction(False)
    try:
        d, _ = sc.render_aa(moved, W, H)
        assert sc.last_render_path() == EXACT
    finally:
        pkg.set_render_prediction(True)
    assert c.tobytes() == d.tobytes()
    assert not np.array_equal(c, a)


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_aa_ranks_merge_into_the_single_rank_frame(pkg, scene_data, nranks):
    sc = _scene(pkg, scene_data, "cornell")
    W, H = 150, 110  # 5 x 4 blocks of 32x32 pixels, the last ones clipped
    cam = pkg.scenes.default_camera(W, H)
    whole, st = sc.render_aa(cam, W, H)
    merged = np.full((W * H, 3), -1.0, np.float32)
    total = 0
    for r in range(nranks):
        _, sr = sc.render_aa(cam, W, H, rank=r, nranks=nranks, rgb=merged)
        total += sr["primary_rays"]
    assert merged.tobytes() == whole.tobytes()
    assert total == st["primary_rays"] == 4 * W * H
    # a rank writes exactly the 32x32 blocks it owns (block index % nranks == rank) and keeps every other pixel
    own = np.full((W * H, 3), -1.0, np.float32)
    sc.render_aa(cam, W, H, rank=1, nranks=nranks, rgb=own)
    bx = (W + 31) // 32
    yy, xx = np.divmod(np.arange(W * H), W)
    mine = ((yy // 32) * bx + xx // 32) % nranks == 1
    assert np.array_equal(own[mine], whole[mine]) and (own[~mine] == -1.0).all()


@pytest.mark.parametrize("nrep", [2, 3])
def test_render_multi_aa_equals_render_aa(pkg, scene_data, nrep):
    sd = scene_data("monkey")
    W, H = 130, 70
    cam = pkg.scenes.default_camera(W, H)
    whole, st = pkg.Scene(sd, device=0).render_aa(cam, W, H)
    reps = [pkg.Scene(sd, device=0) for _ in range(nrep)]
    got, sm = pkg.render_multi_aa(reps, cam, W, H)
    assert got.tobytes() == whole.tobytes()
    assert sm["primary_rays"] == 4 * W * H and sm["shadow_rays"] == st["shadow_rays"]


@pytest.mark.parametrize("name", ["cornell", "monkey"])
def test_mirror_drivers_agree(pkg, scene_data, name):
    """renderToBuffer* with antiAliasing: the device driver, the host wavefront and the reference's loop taken literally (upstream's
    own ndc expression, an independent check of finding AA3) agree within the parity bar."""
    sd = scene_data(name)
    W, H = 40, 30
    cam = pkg.scenes.default_camera(W, H)
    dev, sd_ = pkg.host_render_aa(sd, cam, W, H, driver="device")
    wav, sw = pkg.host_render_aa(sd, cam, W, H, driver="wavefront")
    per, sp = pkg.host_render_aa(sd, cam, W, H, driver="per_ray")
    assert sd_["primary"] == sw["primary"] == sp["primary"] == 4 * W * H
    assert np.abs(dev.astype(np.float64) - wav).max() <= TOL
    assert np.abs(dev.astype(np.float64) - per).max() <= TOL
    assert (dev.sum(1) > 0).mean() > 0.05
    multi, _ = pkg.host_render_aa(sd, cam, W, H, driver="device", nreplicas=2)
    assert multi.tobytes() == dev.tobytes()


def _bmp_from_rgb(rgb, W, H):
    """Screen::setPixel + writeBitmapToFile for an (H*W, 3) float frame (screen.cpp:30-49): clamp, * 255 truncated, BGR, rows
    bottom-up padded to 4 bytes (tests/test_boundary_gpu.py states the same)."""
    img = np.clip(rgb.reshape(H, W, 3).astype(np.float32), 0.0, 1.0)
    u8 = (img * np.float32(255.0)).astype(np.uint8)
    row_bytes = (W * 3 + 3) & ~3
    data = np.zeros((H, row_bytes), np.uint8)
    data[:, :W * 3] = u8[:, :, ::-1].reshape(H, W * 3)
    hdr = bytearray(54)
    hdr[0:2] = b"BM"
    hdr[2:6] = (54 + row_bytes * H).to_bytes(4, "little")
    hdr[10:14] = (54).to_bytes(4, "little")
    hdr[14:18] = (40).to_bytes(4, "little")
    hdr[18:22] = W.to_bytes(4, "little")
    hdr[22:26] = H.to_bytes(4, "little")
    hdr[26:28] = (1).to_bytes(2, "little")
    hdr[28:30] = (24).to_bytes(2, "little")
    hdr[34:38] = (row_bytes * H).to_bytes(4, "little")
    return bytes(hdr) + data.tobytes()


@pytest.mark.parametrize("nrep", [1, 2])
def test_aa_bmp_equals_resolved_oracle_bmp(pkg, orc, scene_data, tmp_path, nrep):
    """`render --aa`'s path (renderRayTracingOnDevice(s) with antiAliasing -> Screen -> writeBitmapToFile): the file equals the BMP of
    the device's own float frame, and the BMP of the oracle's resolved frame except where a channel sits within the parity bar of an
    8-bit truncation boundary."""
    sd = scene_data("cornell")
    W, H = 240, 136
    cam = pkg.scenes.default_camera(W, H)
    path = str(tmp_path / "aa.bmp")
    rgb, _ = pkg.host_render_aa(sd, cam, W, H, driver="device", nreplicas=nrep, path=path)
    got = open(path, "rb").read()
    mine = _bmp_from_rgb(rgb, W, H)
    assert got[:54] == mine[:54], "BMP header differs from the one stated here"
    assert got == mine, "Screen/BMP bytes differ from the device's float frame"
    sub, _ = orc.OracleScene(sd).render(cam, 2 * W, 2 * H, sd.point_lights, max_level=2)
    ref = pkg.resolve_aa(sub, W, H)
    assert np.abs(rgb.astype(np.float64) - ref).max() <= TOL
    want = _bmp_from_rgb(ref, W, H)
    a = np.frombuffer(got, np.uint8)[54:].astype(np.int16)
    b = np.frombuffer(want, np.uint8)[54:].astype(np.int16)
    diff = np.nonzero(a != b)[0]
    v = np.clip(ref.astype(np.float64), 0, 1) * 255.0
    near = np.abs(v - np.round(v)) <= TOL * 255.0 + 1e-9
    assert len(diff) <= near.sum() and np.abs(a - b).max(initial=0) <= 1


def test_render_cli_aa_writes_a_bmp(pkg, tmp_path):
    """`render --aa <data> file.obj W H depth out.bmp` runs and writes a BMP of the frame's size (the CLI's scene presets need the
    reference's data directory, which the suite does not carry; an OBJ fixture stands in)."""
    import subprocess

    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "render")
    obj = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj", "small.obj")
    out = str(tmp_path / "cli.bmp")
    r = subprocess.run([exe, "--aa", str(tmp_path), obj, "33", "17", "2", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    assert data[:2] == b"BM" and int.from_bytes(data[18:22], "little") == 33 and int.from_bytes(data[22:26], "little") == 17
    assert f"{4 * 33 * 17} primary" in r.stdout

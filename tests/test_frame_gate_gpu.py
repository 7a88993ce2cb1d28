"""GPU tests of the frame gate (cgrt_set_frame_gate; capi.cpp frame_gate_rect, trace_kernels.hip wave_outside_gate): waves
whose pixels all lie outside the root box's screen rectangle write their miss records without generating a ray.  Every frame must be
the frame of the per-pixel path -- gate on against gate off, byte for byte -- and both must be the oracle's: flag, t bits, ids, and
normals where hit.  Frames of 200x120 and 97x61 on the smoke scene and on dodge, so that the rectangle cuts through tiles and
super-tiles: plain, a rect sub-frame, two ranks, the packed multi-device order, frame hints forced on, the forced quad shape; the
shaded frame at depth 2 (blocking, predicted, enqueued); the counting kernel; a scene with spheres (never gated)."""
import numpy as np
import pytest

from test_parity_gpu import _assert_hits_equal

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(200, 120), (97, 61)]
SCENES = ["dragon20k", "dodge"]


def _cams(pkg, W, H):
    """The default camera (the box in the middle of the frame) and one that puts it into a corner, cut by the frame's edge."""
    corner = pkg.scenes.default_camera(W, H).copy()
    corner[0:3] = [0.55, 0.35, 0.0]
    return {"default": pkg.scenes.default_camera(W, H), "corner": corner}


@pytest.fixture(scope="module")
def world(pkg, orc, scene_data):
    """name -> (scene data, device scene, ref(cam name, W, H) -> the oracle's hits of the whole frame, computed once)"""
    cache, refs = {}, {}

    def get(name):
        if name not in cache:
            sd = pkg.scenes.make_dragon(20_000) if name == "dragon20k" else scene_data(name)
            cache[name] = (sd, pkg.Scene(sd), orc.OracleScene(sd))

        def ref(cname, W, H):
            key = (name, cname, W, H)
            if key not in refs:
                refs[key] = cache[name][2].intersect(orc.generate_rays(_cams(pkg, W, H)[cname], W, H))
                refs[key].setflags(write=False)
            return refs[key]

        return cache[name][0], cache[name][1], ref

    return get


@pytest.fixture
def gate(pkg):
    yield pkg.set_frame_gate
    pkg.set_frame_gate(True)
    pkg.set_frame_hints(-1)
    pkg.debug_set_hint_thresholds(0, 0)
    pkg.set_kernel_shape(-1)


def _both(gate, call):
    """call() with the gate on and off: the two results, asserted byte-identical (arrays or tuples of arrays / None)."""
    gate(True)
    on = call()
    gate(False)
    off = call()
    gate(True)
    for a, b in zip(on if isinstance(on, tuple) else (on,), off if isinstance(off, tuple) else (off,)):
        if isinstance(a, np.ndarray):
            assert a.tobytes() == b.tobytes(), "gate on and gate off differ"
    return on


def _owned(hits):
    return ~np.isnan(hits["t"])  # (Scene.trace_primary marks what a call does not own; a miss has t = FLT_MAX)


def _assert_owned_equal(hits, normals, ref, owned, what):
    assert owned.any(), what
    _assert_hits_equal(hits[owned], None if normals is None else normals[owned], ref[owned], what)
    rest = hits[~owned]
    assert np.isnan(rest["t"]).all() and (rest["hit"] == 0).all(), f"{what}: a pixel the call does not own was written"


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_gated_frames_equal_ungated_frames_and_the_oracle(pkg, world, gate, name, W, H):
    sd, sc, ref = world(name)
    for cname, cam in _cams(pkg, W, H).items():
        r = sc.frame_gate(cam, W, H)
        assert r is not None and (r[2] - r[0]) * (r[3] - r[1]) < W * H, f"{name} {cname}: the gate has nothing to skip ({r})"
        assert (r[0] % 8 or r[1] % 8 or r[2] % 8 or r[3] % 8), f"{name} {cname}: {r} cuts no tile"
        want = ref(cname, W, H)
        what = f"{name} {W}x{H} {cname}"
        # the plain frame
        h, n = _both(gate, lambda: sc.trace_primary(cam, W, H, want_normals=True))
        _assert_hits_equal(h, n, want, what)
        # rect sub-frames: one across the rectangle's edges, one wholly outside it where there is room
        rects = [(3, 5, W - 10, H - 7), (max(r[0] - 2, 0), max(r[1] - 3, 0), min(r[0] + 21, W), min(r[1] + 13, H))]
        if r[0] >= 2:
            rects.append((0, 0, r[0], H))
        for rect in rects:
            h, n = _both(gate, lambda: sc.trace_primary(cam, W, H, rect=rect, want_normals=True))
            own = np.zeros((H, W), bool)
            own[rect[1]:rect[3], rect[0]:rect[2]] = True
            assert np.array_equal(_owned(h), own.reshape(-1)), f"{what} rect {rect}"
            _assert_owned_equal(h, n, want, own.reshape(-1), f"{what} rect {rect}")
        # rank / nranks = 0/2 and 1/2: each rank its own pixels, together the frame
        parts = [_both(gate, lambda k=k: sc.trace_primary(cam, W, H, rank=k, nranks=2, want_normals=True)) for k in range(2)]
        o0, o1 = _owned(parts[0][0]), _owned(parts[1][0])
        assert not (o0 & o1).any() and (o0 | o1).all(), what
        for k, (h, n) in enumerate(parts):
            _assert_owned_equal(h, n, want, (o0, o1)[k], f"{what} rank {k}/2")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_gated_packed_hinted_and_quad_frames(pkg, world, gate, name, W, H):
    sd, sc, ref = world(name)
    replicas = [sc, pkg.Scene(sd)]
    for cname, cam in _cams(pkg, W, H).items():
        want = ref(cname, W, H)
        what = f"{name} {W}x{H} {cname}"
        # the packed multi-device order (two replicas on one device)
        h, n, _ = _both(gate, lambda: pkg.trace_primary_multi(replicas, cam, W, H, want_normals=True))
        _assert_hits_equal(h, n, want, what + " packed")
        # frame hints forced on, every traced tile hard (20 ticks): frames of one shape one after the other, with the gate on and off
        pkg.debug_set_hint_thresholds(20, 20)
        for mode in (1, 2):
            for on in (True, False):
                gate(on)
                pkg.set_frame_hints(mode)
                for k in range(6):  # (a shape gets its hint buffers at the third frame; then lists are written, read and rotated)
                    h, n = sc.trace_primary(cam, W, H, want_normals=True)
                    _assert_hits_equal(h, n, want, f"{what} hints {mode} gate {on} frame {k}")
                pkg.set_frame_hints(0)
        pkg.set_frame_hints(-1)
        pkg.debug_set_hint_thresholds(0, 0)
        # the forced quad shape
        pkg.set_kernel_shape(1)
        h, n = _both(gate, lambda: sc.trace_primary(cam, W, H, want_normals=True))
        _assert_hits_equal(h, n, want, what + " quad")
        h, n = _both(gate, lambda: sc.trace_primary(cam, W, H, rank=1, nranks=2, want_normals=True))
        _assert_owned_equal(h, n, want, _owned(h), what + " quad rank 1/2")
        pkg.set_kernel_shape(-1)


@pytest.mark.parametrize("name", SCENES)
def test_shaded_frames_and_counters_do_not_depend_on_the_gate(pkg, world, gate, name):
    sd, sc, _ = world(name)
    W, H = 200, 120
    cam = _cams(pkg, W, H)["default"]
    lights = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    if len(lights) == 0:
        lights = np.asarray([[0.0, 2.0, 2.0, 1.0, 1.0, 1.0]], np.float32)
    keys = ("primary_rays", "shadow_rays", "reflection_rays", "levels")
    frames = []
    for on in (True, False, True):
        gate(on)
        for k in range(2):  # (the second frame of a shape is a predicted one: the fused primary kernel)
            rgb, st = sc.render(cam, W, H, lights=lights, max_level=2)
            frames.append((rgb, {q: st[q] for q in keys}))
    for rgb, st in frames[1:]:
        assert rgb.tobytes() == frames[0][0].tobytes() and st == frames[0][1]
    assert frames[0][0].any(), "the frame is not black"
    # the enqueued frame (cgrt_enqueue_render_device) and the quad shape of the fused kernel
    outs = []
    for on in (True, False):
        gate(on)
        out, ticket = sc.enqueue_render_tensor(cam, W, H, lights=lights, max_level=2)
        st = sc.enqueue_stats(ticket)
        outs.append((out.cpu().numpy().copy(), {q: st[q] for q in keys}))
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1] == outs[1][1] == frames[0][1]
    assert outs[0][0].reshape(-1, 3).tobytes() == frames[0][0].tobytes()
    pkg.set_kernel_shape(1)
    quad = _both(gate, lambda: sc.render(cam, W, H, lights=lights, max_level=2)[0])
    pkg.set_kernel_shape(-1)
    assert quad.tobytes() == frames[0][0].tobytes()
    # the counting kernel takes the per-pixel path either way: equal dictionaries, every owned pixel a ray
    for kw in ({}, {"rect": (3, 5, W - 10, H - 7)}, {"rank": 1, "nranks": 2}):
        gate(True)
        c_on = sc.count_primary(cam, W, H, **kw)
        gate(False)
        c_off = sc.count_primary(cam, W, H, **kw)
        assert c_on == c_off, kw
    gate(True)
    assert sc.count_primary(cam, W, H)["rays"] == W * H


def test_a_scene_with_spheres_is_never_gated(pkg, orc, gate):
    sd = pkg.scenes.spheres_preset()
    sc = pkg.Scene(sd)
    o = orc.OracleScene(sd)
    for W, H in SIZES:
        cam = np.asarray([0, 0, 6, 0, 0, 0, 8.0, np.radians(50.0), np.float32(W) / np.float32(H)], np.float32)
        assert sc.frame_gate(cam, W, H) is None
        h, n = _both(gate, lambda: sc.trace_primary(cam, W, H, want_normals=True))
        want = o.intersect(orc.generate_rays(cam, W, H))
        assert want["hit"].any()
        _assert_hits_equal(h, n, want, f"spheres {W}x{H}")

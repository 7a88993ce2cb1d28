"""GPU tests of the geometry buffers of a device frame (include/cgrt.h CgrtAovOut, cgrt_*_aov_device; Scene.render_aov_tensor,
render_views_aov_tensor and their enqueued forms).

Everything is bit for bit: each plane is defined as bytes the library already produces.  depth / prim_id / material_id / mask are the fields
of trace_primary_device's hit records, normal its normals where the mask is 1 and 0 elsewhere, albedo materials[material_id, 0:3] or 0,
position float32(o + float32(d * t)) from Scene.generate_rays and depth where the mask is 1, 0 elsewhere.  All seven planes of a call live
in one arena of sentinel bytes: only the requested planes are handed to the call, and every byte of the arena outside them -- the guards
between the planes, and the slots of the planes that were not requested -- must survive.  Asking for planes changes nothing else: colour
bytes, stats, render path and the next plain frame equal those of the same sequence without planes."""
import copy
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAMES = ("depth", "normal", "position", "albedo", "prim_id", "material_id", "mask")
THREE = ("normal", "position", "albedo")
ELEM = {"depth": 4, "normal": 12, "position": 12, "albedo": 12, "prim_id": 4, "material_id": 4, "mask": 1}
SENTINEL = 0xA5
PAD = 256
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")
FORMATS = ("rgb", "chw", "rgba8")
# each plane alone, every subset size from two to six, and all seven
SUBSETS = [(k,) for k in NAMES] + [NAMES[:k] for k in range(2, 7)] + [("mask", "albedo", "depth"), NAMES]


def _dtype(name):
    return {"prim_id": torch.int32, "material_id": torch.int32, "mask": torch.uint8}.get(name, torch.float32)


def _shape(name, lead, W, H, chw):
    return tuple(lead) + (((3, H, W) if chw else (H, W, 3)) if name in THREE else (H, W))


class Arena:
    """Seven plane slots between guards, filled with the sentinel; planes(subset) are the tensors to hand to a call."""

    def __init__(self, lead, W, H, chw, fill=SENTINEL):
        self.lead, self.W, self.H, self.chw = tuple(lead), W, H, chw
        self.px = int(np.prod(self.lead, dtype=np.int64)) * W * H
        self.off, at = {}, PAD
        for k in NAMES:
            self.off[k] = at
            at += -(-(ELEM[k] * self.px) // PAD) * PAD + PAD
        self.buf = torch.full((at,), fill, dtype=torch.uint8, device="cuda")
        self.fill = fill

    def planes(self, subset):
        return {k: self.buf[self.off[k] : self.off[k] + ELEM[k] * self.px].view(_dtype(k)).view(_shape(k, self.lead, self.W, self.H, self.chw))
                for k in subset}

    def untouched_outside(self, subset):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy().copy()
        for k in subset:
            b[self.off[k] : self.off[k] + ELEM[k] * self.px] = self.fill
        return bool((b == self.fill).all())


def _hw3(name, a, chw):
    """A 3-channel plane as (..., H, W, 3)."""
    return np.moveaxis(a, -3, -1) if (chw and name in THREE) else a


def _np(planes, chw):
    torch.cuda.synchronize()
    return {k: _hw3(k, t.cpu().numpy(), chw) for k, t in planes.items()}


def _reference(pkg, sc, cam, W, H):
    """The planes of cam's W x H frame from the library's own second trace and Scene.generate_rays."""
    h = torch.zeros((W * H * 16,), dtype=torch.uint8, device="cuda")
    n = torch.zeros((W * H * 12,), dtype=torch.uint8, device="cuda")
    sc.trace_primary_device(cam, W, H, h.data_ptr(), d_normals_ptr=n.data_ptr())
    torch.cuda.synchronize()
    hits = h.cpu().numpy().view(pkg.HIT_DTYPE).reshape(H, W)
    normals = n.cpu().numpy().view(np.float32).reshape(H, W, 3)
    return _planes_of(pkg, sc, cam, W, H, hits["t"], hits["prim_id"], hits["material_id"], hits["hit"], normals)


def _planes_of(pkg, sc, cam, W, H, t, prim, material, hit, normals):
    m = (hit != 0).reshape(H, W)
    rays = sc.generate_rays(cam, W, H)
    o = np.ascontiguousarray(rays["origin"], np.float32).reshape(H, W, 3)
    d = np.ascontiguousarray(rays["direction"], np.float32).reshape(H, W, 3)
    depth = np.ascontiguousarray(t, np.float32).reshape(H, W)
    with np.errstate(all="ignore"):
        position = np.float32(o + np.float32(d * depth[..., None]))
    mats = np.asarray(sc.sd.materials, np.float32).reshape(-1, 8)
    mid = np.ascontiguousarray(material, np.int32).reshape(H, W)
    albedo = np.zeros((H, W, 3), np.float32)
    if len(mats):
        albedo[mid >= 0] = mats[mid[mid >= 0], 0:3]
    z3 = np.zeros((H, W, 3), np.float32)
    return {
        "depth": depth,
        "normal": np.where(m[..., None], np.asarray(normals, np.float32).reshape(H, W, 3), z3),
        "position": np.where(m[..., None], position, z3),
        "albedo": albedo,
        "prim_id": np.ascontiguousarray(prim, np.uint32).reshape(H, W),
        "material_id": mid,
        "mask": m.astype(np.uint8),
    }


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _assert_planes(got, ref, what):
    for k, g in got.items():
        r = ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        bad = np.argwhere(_bits(g) != _bits(r))
        assert bad.size == 0, (what, k, f"{len(bad)} elements differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} vs {r[tuple(bad[0])]!r}")


def _share(ref):
    return float(ref["mask"].mean())


def _away(pkg, W, H):
    """A camera that sees nothing: it orbits a point far from the scene."""
    cam = pkg.scenes.default_camera(max(W, 1), max(H, 1)).copy()
    cam[0:3] = 1000.0
    return cam


def _moved(pkg, W, H, i):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[3] += np.float32(0.03 * i)
    cam[4] += np.float32(0.05 * i)
    return cam


def _camera(pkg, W, H, distance=3.0, yaw_deg=20.0):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[4] = np.float32(yaw_deg) * np.float32(0.01745329251994329576923690768489)
    cam[6] = distance
    return cam


def _mirror_cornell(scene_data):
    """The Cornell box with every surface a mirror (ks = 0.5): its ray trees reach every level a frame allows."""
    sd = copy.deepcopy(scene_data("cornell"))
    sd.materials = np.array(sd.materials, np.float32, copy=True)
    sd.materials[:, 3:6] = 0.5
    return sd


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    made = {}

    def get(name):
        if name not in made:
            sd = pkg.scenes.make_dragon(20_000) if name == "dragon" else pkg.scenes.spheres_preset() if name == "spheres" else scene_data(name)
            made[name] = pkg.Scene(sd, device=0)
        return made[name]

    yield get
    for s in made.values():
        s.close()


# ---- 1. the planes against the library's own second trace; 8. sentinels around every plane, unrequested slots untouched ----
@pytest.mark.parametrize("name", ["cube", "monkey", "cornell", "spheres", "dragon"])
def test_planes_equal_the_second_trace(pkg, scenes, name):
    sc = scenes(name)
    cases = [(97, 61, "default"), (1, 1, "default"), (3, 1, "default"), (800, 800, "default"), (97, 61, "away"), (1, 1, "near"), (3, 1, "near")]
    for W, H, which in cases:
        cam = _away(pkg, W, H) if which == "away" else pkg.scenes.default_camera(W, H)
        if which == "near":  # (the tiny frames of the default camera miss everything: the same shapes from close up as well)
            cam = _camera(pkg, W, H, distance=1.5)
        ref = _reference(pkg, sc, cam, W, H)
        share = _share(ref)
        print(f"{name} {W}x{H} {which}: hit share {share:.4f}")
        if which == "away":
            assert share == 0.0, "the camera that sees nothing sees something"
        elif W * H > 3:
            assert 0.05 <= share <= 0.95, (name, W, H, share)
        if name == "spheres" and W * H > 3:
            hit = ref["mask"] == 1
            assert (ref["material_id"][hit] == -1).all() and (ref["prim_id"][hit] >= sc.sd.ntris).all() and not ref["albedo"].any()
        plain, st_plain = sc.render_tensor(cam, W, H, max_level=2)
        plain = plain.clone()
        for chw in (False, True):
            for subset in SUBSETS:
                arena = Arena((), W, H, chw)
                out, st, planes = sc.render_aov_tensor(cam, W, H, aovs=subset, chw=chw, aov_out=arena.planes(subset), max_level=2)
                assert set(planes) == set(subset)
                _assert_planes(_np(planes, chw), ref, (name, W, H, which, chw, subset))
                assert arena.untouched_outside(subset), (name, W, H, which, chw, subset, "bytes outside the requested planes were written")
                assert torch.equal(out, plain) and all(st[k] == st_plain[k] for k in KEYS)
    # new tensors when the caller supplies none: shapes and dtypes as documented
    W, H = 97, 61
    cam = pkg.scenes.default_camera(W, H)
    ref = _reference(pkg, sc, cam, W, H)
    for chw in (False, True):
        _, _, planes = sc.render_aov_tensor(cam, W, H, chw=chw)
        assert tuple(planes) == NAMES
        for k, t in planes.items():
            assert t.dtype == _dtype(k) and tuple(t.shape) == _shape(k, (), W, H, chw) and t.is_contiguous()
        _assert_planes(_np(planes, chw), ref, (name, "new tensors", chw))


# ---- 2. against the CPU oracle ----
@pytest.mark.parametrize("name", ["monkey", "cornell"])
def test_planes_equal_the_oracle(pkg, orc, scenes, name):
    sc = scenes(name)
    W, H = 97, 61
    cam = pkg.scenes.default_camera(W, H)
    o = orc.OracleScene(sc.sd).intersect(sc.generate_rays(cam, W, H))
    ref = _planes_of(pkg, sc, cam, W, H, o["t"], o["prim"], o["material"], o["hit"], o["normal"])
    assert 0.05 <= _share(ref) <= 0.95
    for chw in (False, True):
        _, _, planes = sc.render_aov_tensor(cam, W, H, chw=chw, max_level=2)
        _assert_planes(_np(planes, chw), ref, (name, "oracle", chw))


# ---- 3. nothing else moves ----
@pytest.mark.parametrize("predict", [True, False])
def test_asking_for_planes_changes_nothing_else(pkg, scene_data, predict):
    sd = scene_data("cornell")
    W, H = 400, 300
    far, near = _camera(pkg, W, H, distance=12.0), _camera(pkg, W, H, distance=2.0)
    cams = [far, far, far, near, near, far]  # first, second and third frame of a shape; a jump the prediction cannot follow; and back
    pkg.set_render_prediction(predict)
    try:
        for fmt in FORMATS:
            a, b, r = pkg.Scene(sd), pkg.Scene(sd), pkg.Scene(sd)  # (r: the second trace, kept off the two scenes under comparison)
            paths = []
            for i, cam in enumerate(cams):
                ref = _reference(pkg, r, cam, W, H)
                oa, sa = a.render_tensor(cam, W, H, format=fmt, max_level=4)
                ob, sb, planes = b.render_aov_tensor(cam, W, H, format=fmt, max_level=4)
                torch.cuda.synchronize()
                assert torch.equal(oa, ob), (fmt, i, "colour bytes")
                assert all(sa[k] == sb[k] for k in KEYS), (fmt, i, sa, sb)
                assert a.last_render_path() == b.last_render_path(), (fmt, i)
                paths.append(b.last_render_path())
                _assert_planes(_np(planes, False), ref, (fmt, i, "planes of the frame that was kept"))
                # the next plain frame on both scenes
                na, ta = a.render_tensor(_moved(pkg, W, H, i), W, H, format=fmt, max_level=4)
                nb, tb = b.render_tensor(_moved(pkg, W, H, i), W, H, format=fmt, max_level=4)
                torch.cuda.synchronize()
                assert torch.equal(na, nb) and all(ta[k] == tb[k] for k in KEYS) and a.last_render_path() == b.last_render_path(), (fmt, i)
            if predict and fmt == "rgb":
                assert 2 in paths, paths  # (the jump was redrawn on the exact path, and the planes came from the redrawn frame)
            for x in (a, b, r):
                x.close()
        # the same camera again and again, and the jump, without frames in between: the paths are the ones the prediction tests name
        b = pkg.Scene(sd)
        seq = []
        for cam in (far, far, far, near):
            ref = _reference(pkg, b, cam, W, H)
            _, _, planes = b.render_aov_tensor(cam, W, H, max_level=4)
            seq.append(b.last_render_path())
            _assert_planes(_np(planes, False), ref, ("sequence", len(seq)))
        assert seq == ([0, 1, 1, 2] if predict else [0, 0, 0, 0]), seq
        b.close()
    finally:
        pkg.set_render_prediction(True)


# ---- 4. deep frames: level 0's buffers must not be recycled under the planes ----
@pytest.mark.parametrize("depth", [4, 6])
@pytest.mark.parametrize("how", ["blocking", "enqueued"])
def test_deep_frames(pkg, scene_data, depth, how):
    W, H = 320, 240
    cam = _camera(pkg, W, H, distance=3.0, yaw_deg=20.0)
    soft = dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(4096, 3), samples=16, seed=11)
    for label, sd in (("cornell", scene_data("cornell")), ("all-mirror cornell", _mirror_cornell(scene_data))):
        sc = pkg.Scene(sd)
        ref = _reference(pkg, sc, cam, W, H)
        assert 0.05 <= _share(ref) <= 0.95
        for kw in ({}, soft):
            plain, st_plain = sc.render_tensor(cam, W, H, max_level=depth, **kw)
            plain = plain.clone()
            if label != "cornell":  # (the fixture's single mirror ends every path at level 1; here level 2 writes mirror rays, level 3 reads them)
                assert st_plain["levels"] >= 4, st_plain
            for rep in range(3):  # (exact, then predicted where the frame can be)
                for chw in (False, True):
                    arena = Arena((), W, H, chw)
                    if how == "blocking":
                        out, st, planes = sc.render_aov_tensor(cam, W, H, chw=chw, aov_out=arena.planes(NAMES), max_level=depth, **kw)
                    else:
                        out, t, planes = sc.enqueue_render_aov_tensor(cam, W, H, chw=chw, aov_out=arena.planes(NAMES), max_level=depth, **kw)
                        st = sc.enqueue_stats(t)
                    _assert_planes(_np(planes, chw), ref, (label, depth, how, bool(kw), rep, chw))
                    assert arena.untouched_outside(NAMES)
                    assert torch.equal(out, plain) and all(st[k] == st_plain[k] for k in KEYS), (label, depth, how, bool(kw), rep)
        sc.close()


# ---- 5. ranks and anti-aliasing ----
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("how", ["blocking", "enqueued"])
def test_ranks_merge_and_leave_other_pixels_alone(pkg, scenes, nranks, how):
    sc = scenes("monkey")
    W, H = 200, 150  # 4 x 3 super-tiles, the last column and row partial
    cam = pkg.scenes.default_camera(W, H)
    ref = _reference(pkg, sc, cam, W, H)
    assert 0.05 <= _share(ref) <= 0.95
    owner = ((np.arange(H)[:, None] // 64) * ((W + 63) // 64) + (np.arange(W)[None, :] // 64)) % nranks
    for chw in (False, True):
        merged = {k: np.full(_shape(k, (), W, H, False), SENTINEL, np.uint8 if k == "mask" else np.uint32) for k in NAMES}
        for rank in range(nranks):
            arena = Arena((), W, H, chw)
            colour = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
            if how == "blocking":
                sc.render_aov_tensor(cam, W, H, chw=chw, out=colour, aov_out=arena.planes(NAMES), max_level=2, rank=rank, nranks=nranks)
            else:
                sc.enqueue_render_aov_tensor(cam, W, H, chw=chw, out=colour, aov_out=arena.planes(NAMES), max_level=2, rank=rank, nranks=nranks)
            assert arena.untouched_outside(NAMES)
            got = _np(arena.planes(NAMES), chw)
            mine = owner == rank
            for k in NAMES:
                g = _bits(got[k])
                sent = np.uint8(SENTINEL) if k == "mask" else np.uint32(0xA5A5A5A5)
                assert (g[~mine] == sent).all(), (k, rank, "a pixel of another rank was written")
                assert (g[mine] == _bits(ref[k])[mine]).all(), (k, rank)
                merged[k][mine] = g[mine]
        for k in NAMES:
            assert (merged[k] == _bits(ref[k])).all(), k


def test_aa_planes_are_the_sub_sample_frame(pkg, scenes):
    sc = scenes("monkey")
    W, H = 97, 61
    cam = pkg.scenes.default_camera(W, H)
    ref = _reference(pkg, sc, cam, 2 * W, 2 * H)
    assert 0.05 <= _share(ref) <= 0.95
    plain_aa, st_aa = sc.render_tensor(cam, W, H, aa=True, max_level=2)
    plain_aa = plain_aa.clone()
    for chw in (False, True):
        _, _, big = sc.render_aov_tensor(cam, 2 * W, 2 * H, chw=chw, max_level=2)
        big = _np(big, chw)
        for enq in (False, True):
            arena = Arena((), 2 * W, 2 * H, chw)
            f = sc.enqueue_render_aov_tensor if enq else sc.render_aov_tensor
            out, _, planes = f(cam, W, H, chw=chw, aa=True, aov_out=arena.planes(NAMES), max_level=2)
            got = _np(planes, chw)
            _assert_planes(got, big, ("aa against the plain 2W x 2H call", chw, enq))
            _assert_planes(got, ref, ("aa against the second trace", chw, enq))
            assert arena.untouched_outside(NAMES)
            assert tuple(out.shape) == (H, W, 3) and torch.equal(out, plain_aa)
    for f in (sc.render_aov_tensor, sc.enqueue_render_aov_tensor):
        with pytest.raises(pkg.CgrtError) as e:
            f(cam, W, H, aa=True, rank=0, nranks=2)
        assert e.value.code == -1


# ---- 6. views ----
@pytest.mark.parametrize("B", [1, 5, 16])
def test_views_equal_single_cameras(pkg, scenes, B):
    sc = scenes("dragon")
    W, H = 97, 61
    cams = np.stack([_moved(pkg, W, H, i) for i in range(B)])
    singles = []
    for b in range(B):
        _, _, p = sc.render_aov_tensor(cams[b], W, H, max_level=2)
        singles.append(_np(p, False))
        ref = _reference(pkg, sc, cams[b], W, H)
        assert 0.05 <= _share(ref) <= 0.95
        _assert_planes(singles[b], ref, ("single", b))
    plain, st_plain = sc.render_views_tensor(cams, W, H, max_level=2)
    plain = plain.clone()
    for chw in (False, True):
        for subset in (NAMES, ("depth",), ("normal", "mask")):
            for enq in (False, True):
                arena = Arena((B,), W, H, chw)
                if enq:
                    out, t, planes = sc.enqueue_render_views_aov_tensor(cams, W, H, aovs=subset, chw=chw, aov_out=arena.planes(subset), max_level=2)
                    st = sc.enqueue_stats(t)
                else:
                    out, st, planes = sc.render_views_aov_tensor(cams, W, H, aovs=subset, chw=chw, aov_out=arena.planes(subset), max_level=2)
                got = _np(planes, chw)
                for k in subset:
                    assert got[k].shape[0] == B
                    for b in range(B):
                        assert (_bits(got[k][b]) == _bits(singles[b][k])).all(), (k, b, chw, enq)
                assert arena.untouched_outside(subset)
                assert torch.equal(out, plain) and all(st[k] == st_plain[k] for k in KEYS)


# ---- 7. enqueued forms ----
@pytest.mark.parametrize("name", ["cube", "cornell", "spheres"])
def test_enqueued_bytes_equal_blocking(pkg, scenes, name):
    sc = scenes(name)
    for W, H in ((97, 61), (1, 1), (3, 1), (320, 200)):
        cam = pkg.scenes.default_camera(W, H)
        for depth in (1, 2, 3):
            for chw in (False, True):
                for subset in (NAMES, ("position",), ("prim_id", "mask")):
                    a1, a2 = Arena((), W, H, chw), Arena((), W, H, chw)
                    ob, sb, pb = sc.render_aov_tensor(cam, W, H, aovs=subset, chw=chw, aov_out=a1.planes(subset), max_level=depth)
                    oe, t, pe = sc.enqueue_render_aov_tensor(cam, W, H, aovs=subset, chw=chw, aov_out=a2.planes(subset), max_level=depth)
                    est = sc.enqueue_stats(t)
                    torch.cuda.synchronize()
                    assert torch.equal(a1.buf, a2.buf), (name, W, H, depth, chw, subset)
                    assert a2.untouched_outside(subset)
                    assert torch.equal(ob, oe) and all(est[k] == sb[k] for k in KEYS)
                    plain_t = sc.enqueue_render_tensor(cam, W, H, max_level=depth)[1]
                    assert all(sc.enqueue_stats(plain_t)[k] == est[k] for k in KEYS), "enqueue_stats with and without planes"


def test_many_frames_in_flight_each_with_its_own_planes(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"), device=0)
    W, H = 96, 80
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    frames = []
    for i in range(20):
        s = streams[i % 2]
        chw = bool(i & 2)
        with torch.cuda.stream(s):
            arena = Arena((), W, H, chw)
            arena.buf.record_stream(s)
            o = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
            o.record_stream(s)
        if i % 5 == 3:  # (a blocking frame with planes among them)
            sc.render_aov_tensor(_moved(pkg, W, H, i), W, H, chw=chw, out=o, aov_out=arena.planes(NAMES), stream=s, max_level=3)
        else:
            sc.enqueue_render_aov_tensor(_moved(pkg, W, H, i), W, H, chw=chw, out=o, aov_out=arena.planes(NAMES), stream=s, max_level=3)
        frames.append((i, chw, arena, o))
    torch.cuda.synchronize()
    for i, chw, arena, o in frames:
        cam = _moved(pkg, W, H, i)
        ref = _reference(pkg, sc, cam, W, H)
        _assert_planes(_np(arena.planes(NAMES), chw), ref, ("in flight", i))
        assert arena.untouched_outside(NAMES)
        plain, _ = sc.render_tensor(cam, W, H, max_level=3)
        torch.cuda.synchronize()
        assert torch.equal(o, plain), i
    sc.close()


def _sleep_cycles(seconds):
    return int(seconds * 1e9 * 2.4)  # (~2.4 GHz shader clock; only the order of magnitude matters)


@pytest.mark.parametrize("kind", ["frame", "views"])
def test_enqueued_planes_order_themselves_behind_the_stream(pkg, scenes, kind):
    sc = scenes("cornell")
    W, H = 128, 96
    cam = pkg.scenes.default_camera(W, H)
    cams = np.stack([_moved(pkg, W, H, i) for i in range(3)])
    lead = (3,) if kind == "views" else ()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        arena, warm = Arena(lead, W, H, False), Arena(lead, W, H, False)
        out = torch.empty(lead + (H, W, 3), dtype=torch.float32, device="cuda")

    def call(ar):
        if kind == "frame":
            return sc.enqueue_render_aov_tensor(cam, W, H, out=out, aov_out=ar.planes(NAMES), stream=s, max_level=3)
        return sc.enqueue_render_views_aov_tensor(cams, W, H, out=out, aov_out=ar.planes(NAMES), stream=s, max_level=3)

    for _ in range(8):  # (warm: the workspace and each of the scene's 8 ticket slots have their size; and the reference bytes)
        call(warm)
    s.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(_sleep_cycles(0.2))
        arena.buf.fill_(0x3C)  # (still to run when the call returns: the planes must land on top of it, the rest keeps it)
        arena.fill = 0x3C
        t0 = time.perf_counter()
        call(arena)
        dt = time.perf_counter() - t0
        ev = torch.cuda.Event()
        ev.record(s)
    pending = not ev.query()
    s.synchronize()
    assert dt < 0.05, f"the enqueue call took {dt * 1e3:.1f} ms"
    assert pending, "the stream had finished when the call returned"
    for k, t in arena.planes(NAMES).items():
        assert torch.equal(t, warm.planes(NAMES)[k]), (k, "the planes did not run behind the fill")
    assert arena.untouched_outside(NAMES)

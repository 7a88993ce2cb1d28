"""GPU tests of ray cameras (include/cgrt.h CgrtRayCamera; Scene.generate_rays_raycam / trace_raycams_device / render_raycams_device /
render_raycams_tensor / enqueue_render_raycams_tensor), DESIGN.md section 5.18.

The expected rays come from the numpy float32 restatement of the header's formula (tests/raycam_ref.py).  Everything behind the rays is
compared with what the library and the CPU oracle give for those rays as a ray list: hits and normals bit for bit, frames bit for bit
against shade_rays_device (a list hashes its soft-shadow draws with p = i, the row-major pixel, as a frame does) and within the project's
RGB bar of 1e-5 of oracle.shade_rays.  Tiles assembled equal the full frame, the geometry planes equal the traced fields, the enqueued and
light-set forms equal the blocking single-set form, and a batch leaves the scene's prediction record and frame hints alone.

Scenes: cornell, monkey, blob, spheres, make_dragon(20_000); both walks where the scene has a fast tree; frame sizes that are not
multiples of 64 and the forced quad shape; a pinhole with an off-centre principal point, an orthographic camera, a camera with origin_d*
and dir_d* together, and a batch that mixes them with different offsets."""
import numpy as np
import pytest

import raycam_ref as R
from conftest import same_bits as _same_bits_elementwise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SCENES = ("cornell", "monkey", "blob", "spheres", "dragon")
FORMATS = ("rgb", "chw", "rgba8")
SIZES = ((67, 45), (200, 130))  # neither a multiple of 64 (nor of the 8x8 tile)
STAT_KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")
AOVS = ("depth", "normal", "position", "albedo", "prim_id", "material_id", "mask")
ELEM = {"depth": 4, "normal": 12, "position": 12, "albedo": 12, "prim_id": 4, "material_id": 4, "mask": 1}
SENTINEL = 0xA5
EXACT, PREDICTED = 0, 1
RGB_BAR = 1e-5  # the project's bar for RGB against the oracle


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and bool(_same_bits_elementwise(a, b).all())


@pytest.fixture(scope="module")
def world(pkg, orc, scene_data):
    """name -> (SceneData, Scene, OracleScene), made once."""
    cache = {}

    def get(name):
        if name not in cache:
            sd = pkg.scenes.make_dragon(20_000) if name == "dragon" else scene_data(name)
            cache[name] = (sd, pkg.Scene(sd), orc.OracleScene(sd))
        return cache[name]

    yield get
    for _, sc, o in cache.values():
        sc.close()
        o.close()


def _walks(sc):
    return (True, False) if sc.build_info()["fast_tree"] else (False,)


def _set_walk(sc, certified):
    if sc.build_info()["fast_tree"]:
        sc.set_walk(certified)


def _cams(pkg, name, W, H):
    """The three kinds, then the mixed batch with offsets: 8 cameras."""
    where = R.WHERE.get(name, {})
    return list(R.camera_set(pkg, W, H, **where).values()) + R.mixed_batch(pkg, W, H, **where)


def _guarded(nbytes, pad=256):
    buf = torch.full((nbytes + 2 * pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    inner = buf[pad : pad + nbytes]

    def intact():
        torch.cuda.synchronize()
        b = buf.cpu().numpy()
        return bool((b[:pad] == SENTINEL).all() and (b[pad + nbytes :] == SENTINEL).all())

    return buf, inner, intact


def _trace(pkg, sc, cams, W, H):
    """(hits (B, W*H) HIT_DTYPE, normals (B, W*H, 3) f32 over a sentinel fill) of trace_raycams_device."""
    B = len(cams)
    hb, hi, hok = _guarded(B * W * H * 16)
    nb, ni, nok = _guarded(B * W * H * 12)
    sc.trace_raycams_device(cams, W, H, hi.data_ptr(), d_normals_ptr=ni.data_ptr())
    assert hok() and nok(), "bytes outside the batch's hits / normals were written"
    return hi.cpu().numpy().view(pkg.HIT_DTYPE).reshape(B, W * H), ni.cpu().numpy().view(np.float32).reshape(B, W * H, 3)


def _intersect_list(pkg, sc, rays):
    """intersect_device on a ray list: (hits, normals over the same sentinel fill)."""
    n = len(rays)
    d = torch.from_numpy(np.ascontiguousarray(rays.view(np.float32).reshape(-1, 7))).cuda()
    h = torch.full((n * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    nn = torch.full((n * 12,), SENTINEL, dtype=torch.uint8, device="cuda")
    sc.intersect_device(d.data_ptr(), n, h.data_ptr(), d_normals_ptr=nn.data_ptr())
    torch.cuda.synchronize()
    return h.cpu().numpy().view(pkg.HIT_DTYPE), nn.cpu().numpy().view(np.float32).reshape(n, 3)


def test_generated_rays_equal_the_restatement(pkg, world):
    sd, sc, _ = world("cornell")
    for W, H in ((1, 1), (5, 3), (64, 64)) + SIZES:
        for name in ("cornell", "spheres"):
            for i, cam in enumerate(_cams(pkg, name, W, H)):
                got = sc.generate_rays_raycam(cam, W, H).view(np.float32).reshape(-1, 7)
                want = R.rays_of(cam, W, H)
                assert np.isfinite(want).all()
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (W, H, name, i)
    # a pixel whose unnormalised direction is zero gets the formula's NaN direction
    cam = pkg.RayCamera.from_fields((0, 0, 0), (0, 0, 0), (0, 0, 0), (-2, 0, 0), (1, 0, 0), (0, 0, 0))
    got = sc.generate_rays_raycam(cam, 5, 1).view(np.float32).reshape(-1, 7)
    assert np.isnan(got[2, 3:6]).all() and same_bits(got, R.rays_of(cam, 5, 1))
    assert np.array_equal(got[[0, 4], 3:6], np.float32([[-1, 0, 0], [1, 0, 0]]))


@pytest.mark.parametrize("name", SCENES)
def test_primary_hits(pkg, world, name):
    sd, sc, o = world(name)
    try:
        for certified in _walks(sc):
            _set_walk(sc, certified)
            for W, H in SIZES:
                shapes = (-1, 1) if (certified and (W, H) == SIZES[0]) else (-1,)  # 1: quad16, taken by scenes with a fast tree
                cams = _cams(pkg, name, W, H)
                rays = [sc.generate_rays_raycam(c, W, H) for c in cams]
                want = [o.intersect(r) for r in rays]
                assert sum(int(w["hit"].sum()) for w in want) > 0.05 * len(cams) * W * H, "the cameras see the scene"
                for shape in shapes:
                    pkg.set_kernel_shape(shape)
                    tag = (name, certified, W, H, shape)
                    hits, normals = _trace(pkg, sc, cams, W, H)
                    for b, cam in enumerate(cams):
                        lh, ln = _intersect_list(pkg, sc, rays[b])
                        assert hits[b].tobytes() == lh.tobytes(), ("hits vs intersect_device", tag, b)
                        assert normals[b].tobytes() == ln.tobytes(), ("normals vs intersect_device", tag, b)
                        w = want[b]
                        assert np.array_equal(hits[b]["hit"], w["hit"]), ("hit", tag, b)
                        assert np.array_equal(hits[b]["t"].view(np.uint32), w["t"].view(np.uint32)), ("t bits", tag, b)
                        assert np.array_equal(hits[b]["prim_id"], w["prim"]), ("prim", tag, b)
                        assert np.array_equal(hits[b]["material_id"], w["material"]), ("material", tag, b)
                        m = w["hit"] == 1
                        assert same_bits(normals[b][m], w["normal"][m]), ("normals of hits", tag, b)
                        if b in (0, 4, 7):  # view b of the batch is the one-view call of cams[b]
                            h1, n1 = _trace(pkg, sc, [cam], W, H)
                            assert h1[0].tobytes() == hits[b].tobytes() and n1[0].tobytes() == normals[b].tobytes(), ("one view", tag, b)
    finally:
        pkg.set_kernel_shape(-1)
        _set_walk(sc, True)


def _as_format(pkg, rgb, W, H, fmt):
    """A (W*H, 3) float32 ray-list frame in the layout of `fmt`."""
    if fmt == "rgb":
        return rgb.reshape(H, W, 3)
    if fmt == "chw":
        return np.ascontiguousarray(rgb.reshape(H, W, 3).transpose(2, 0, 1))
    return pkg.rgba8_of(rgb, W, H)


def _shade_list(sc, rays, **kw):
    d = torch.from_numpy(np.ascontiguousarray(rays.view(np.float32).reshape(-1, 7))).cuda()
    out, st = sc.shade_rays_tensor(d, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), st


def _oracle_check(o, rays, got, lights, tag, **kw):
    want, wc = o.shade_rays(rays, lights, threads=16, **kw)
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    eq = _same_bits_elementwise(got, want)
    with np.errstate(invalid="ignore"):
        err = np.where(eq, 0.0, np.abs(got.astype(np.float64) - want))
    worst = float(np.nanmax(err, initial=0.0))
    print("rgb error against the oracle", tag, worst)
    assert not np.isnan(err).any() and worst <= RGB_BAR, (tag, worst)
    return wc


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("depth", [0, 1, 2, 4])
def test_frames_point_lights(pkg, world, name, depth):
    sd, sc, o = world(name)
    lights = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    try:
        for certified in _walks(sc):
            _set_walk(sc, certified)
            for W, H in SIZES if depth == 2 else SIZES[:1]:
                shapes = (-1, 1) if (certified and depth == 2 and (W, H) == SIZES[0]) else (-1,)
                cams = _cams(pkg, name, W, H)
                rays = [sc.generate_rays_raycam(c, W, H) for c in cams]
                lists = [_shade_list(sc, r, max_level=depth) for r in rays]
                for shape in shapes:
                    pkg.set_kernel_shape(shape)
                    for fmt in FORMATS:
                        t, st = sc.render_raycams_tensor(cams, W, H, format=fmt, max_level=depth)
                        torch.cuda.synchronize()
                        a = t.cpu().numpy()
                        for b in range(len(cams)):
                            assert a[b].tobytes() == _as_format(pkg, lists[b][0], W, H, fmt).tobytes(), (name, certified, W, H, shape, fmt, b)
                        for k in STAT_KEYS[:4]:
                            assert st[k] == sum(ls[1][k] for ls in lists), (k, fmt)
                if not certified or len(_walks(sc)) == 1:  # (the frames of both walks are the same bytes: the oracle once)
                    t, _ = sc.render_raycams_tensor(cams, W, H, format="rgb", max_level=depth)
                    torch.cuda.synchronize()
                    a = t.cpu().numpy().reshape(len(cams), W * H, 3)
                    for b in (0, 1, 2, 6):
                        _oracle_check(o, rays[b], a[b], lights, (name, depth, W, H, b), max_level=depth)
                    if depth and name != "spheres":  # (the preset's spheres carry no material: they shade black)
                        assert a.any(), "something is lit"
    finally:
        pkg.set_kernel_shape(-1)
        _set_walk(sc, True)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("depth", [1, 2, 4])
def test_frames_spherical_lights(pkg, world, name, depth):
    """Sample smp of pixel (x, y) of view b is hashed with y*W + x -- the index of that ray in the view's row-major list."""
    sd, sc, o = world(name)
    lights = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    where = R.WHERE.get(name, {})
    sph = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
    sph[:, 0:3] = sph[:, 0:3] * np.float32(where.get("scale", 1.0)) + np.asarray(where.get("at", (0, 0, 0)), np.float32)
    soft = dict(spherical=sph, units=pkg.unit_vector_table(1000, 5), samples=6, seed=123)
    W, H = 61, 37
    cams = _cams(pkg, name, W, H)
    rays = [sc.generate_rays_raycam(c, W, H) for c in cams]
    try:
        for certified in _walks(sc):
            _set_walk(sc, certified)
            lists = [_shade_list(sc, r, lights=lights, max_level=depth, **soft) for r in rays]
            for fmt in FORMATS:
                t, st = sc.render_raycams_tensor(cams, W, H, format=fmt, lights=lights, max_level=depth, **soft)
                torch.cuda.synchronize()
                a = t.cpu().numpy()
                for b in range(len(cams)):
                    assert a[b].tobytes() == _as_format(pkg, lists[b][0], W, H, fmt).tobytes(), (name, certified, depth, fmt, b)
                for k in STAT_KEYS[:4]:
                    assert st[k] == sum(ls[1][k] for ls in lists), (k, fmt)
                assert st["soft_shadow_rays"] > 0
        for b in (0, 1, 2, 6):
            wc = _oracle_check(o, rays[b], lists[b][0], lights, (name, "soft", depth, b), max_level=depth, **soft)
            for k in STAT_KEYS[:4]:
                assert lists[b][1][k] == wc[k], (k, b)
    finally:
        _set_walk(sc, True)


def _planes_ref(pkg, sd, hits, normals, rays, W, H):
    """The seven planes from the fields trace_raycams_device returns for the camera (hits (W*H,), normals over any fill) and its rays."""
    m = hits["hit"] == 1
    r = rays.view(np.float32).reshape(-1, 7)
    depth = hits["t"].copy()
    z3 = np.zeros((W * H, 3), np.float32)
    with np.errstate(all="ignore"):
        position = np.float32(r[:, 0:3] + np.float32(r[:, 3:6] * depth[:, None]))
    mats = np.asarray(sd.materials, np.float32).reshape(-1, 8)
    mid = hits["material_id"]
    albedo = z3.copy()
    albedo[mid >= 0] = mats[mid[mid >= 0], 0:3]
    return {
        "depth": depth.reshape(H, W),
        "normal": np.where(m[:, None], normals, z3).reshape(H, W, 3),
        "position": np.where(m[:, None], position, z3).reshape(H, W, 3),
        "albedo": albedo.reshape(H, W, 3),
        "prim_id": hits["prim_id"].view(np.int32).reshape(H, W),
        "material_id": mid.reshape(H, W),
        "mask": hits["hit"].astype(np.uint8).reshape(H, W),
    }


@pytest.mark.parametrize("name", ["cornell", "spheres", "dragon"])
@pytest.mark.parametrize("chw", [False, True])
def test_geometry_planes(pkg, world, name, chw):
    sd, sc, _ = world(name)
    W, H = SIZES[0]
    cams = _cams(pkg, name, W, H)
    B = len(cams)
    hits, normals = _trace(pkg, sc, cams, W, H)
    ob, oi, ook = _guarded(B * W * H * 12)
    guards = {k: _guarded(B * W * H * ELEM[k]) for k in AOVS}
    st = sc.render_raycams_device(cams, W, H, oi.data_ptr(), aov={k: g[1].data_ptr() for k, g in guards.items()}, chw=chw, max_level=2)
    assert ook() and all(g[2]() for g in guards.values()), "bytes outside an output were written"
    plain, st0 = sc.render_raycams_tensor(cams, W, H, max_level=2)
    torch.cuda.synchronize()
    assert oi.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), "the colour does not depend on the planes"
    assert all(st[k] == st0[k] for k in STAT_KEYS)
    dt = {"depth": np.float32, "normal": np.float32, "position": np.float32, "albedo": np.float32, "prim_id": np.int32, "material_id": np.int32,
          "mask": np.uint8}
    got = {k: guards[k][1].cpu().numpy().view(dt[k]) for k in AOVS}
    for b, cam in enumerate(cams):
        ref = _planes_ref(pkg, sd, hits[b], normals[b], sc.generate_rays_raycam(cam, W, H), W, H)
        for k in AOVS:
            want = ref[k]
            if chw and want.ndim == 3:
                want = np.ascontiguousarray(want.transpose(2, 0, 1))
            g = got[k].reshape((B,) + want.shape)[b]
            ok = same_bits(g, want) if dt[k] == np.float32 else np.array_equal(g, want)
            assert ok, (name, chw, k, b)
    # the tensor form returns the same planes
    t, st1, planes = sc.render_raycams_tensor(cams, W, H, aovs=AOVS, chw=chw, max_level=2)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    for k in AOVS:
        assert planes[k].cpu().numpy().tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("name", ["cornell", "dragon", "spheres"])
def test_tiles_assemble_to_the_full_frame(pkg, world, name):
    """Four tiles of a frame, each a call of its own with the tile's offsets: hits, every geometry plane and RGB under point lights."""
    sd, sc, _ = world(name)
    W, H, X, Y = 150, 101, 64, 50
    where = R.WHERE.get(name, {})
    try:
        for certified in _walks(sc):
            _set_walk(sc, certified)
            for kind, cam in R.camera_set(pkg, W, H, **where).items():
                cam = cam.tile(-11, 5)  # (a camera that already carries offsets)
                fh, fn = _trace(pkg, sc, [cam], W, H)
                for fmt in ("rgb", "rgba8"):
                    full, _, fplanes = sc.render_raycams_tensor(cam, W, H, format=fmt, aovs=AOVS, max_level=2)
                    torch.cuda.synchronize()
                    full = full.cpu().numpy()[0]
                    asm = np.zeros_like(full)
                    aplanes = {k: np.zeros_like(v.cpu().numpy()[0]) for k, v in fplanes.items()}
                    ah, an = np.zeros((H, W), pkg.HIT_DTYPE), np.zeros((H, W, 3), np.float32)
                    for x0, y0, w, h in ((0, 0, X, Y), (X, 0, W - X, Y), (0, Y, X, H - Y), (X, Y, W - X, H - Y)):
                        tc = cam.tile(x0, y0)
                        t, _, planes = sc.render_raycams_tensor(tc, w, h, format=fmt, aovs=AOVS, max_level=2)
                        torch.cuda.synchronize()
                        rows = slice(H - y0 - h, H - y0) if fmt == "rgba8" else slice(y0, y0 + h)  # (rgba8 is the bitmap: bottom row first)
                        asm[rows, x0 : x0 + w] = t.cpu().numpy()[0]
                        for k in AOVS:
                            aplanes[k][y0 : y0 + h, x0 : x0 + w] = planes[k].cpu().numpy()[0]
                        th, tn = _trace(pkg, sc, [tc], w, h)
                        ah[y0 : y0 + h, x0 : x0 + w] = th[0].reshape(h, w)
                        an[y0 : y0 + h, x0 : x0 + w] = tn[0].reshape(h, w, 3)
                    tag = (name, certified, kind, fmt)
                    assert asm.tobytes() == full.tobytes(), ("rgb", tag)
                    for k in AOVS:
                        assert aplanes[k].tobytes() == fplanes[k].cpu().numpy()[0].tobytes(), (k, tag)
                    assert ah.tobytes() == fh[0].tobytes(), ("hits", tag)
                    hit = fh[0]["hit"].reshape(H, W) == 1
                    assert an[hit].tobytes() == fn[0].reshape(H, W, 3)[hit].tobytes(), ("normals", tag)
                    assert hit.any() and (full.any() or name == "spheres")  # (spheres carry no material: they shade black)
    finally:
        _set_walk(sc, True)


def test_enqueued_form(pkg, world):
    sd, sc, _ = world("cornell")
    W, H = 200, 130
    cams = _cams(pkg, "cornell", W, H)
    B = len(cams)
    soft = dict(spherical=pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy(), units=pkg.unit_vector_table(1000, 5), samples=4, seed=9)
    for kw in (dict(max_level=2), dict(max_level=4), dict(max_level=0), dict(max_level=2, **soft)):
        for fmt in FORMATS:
            ref, rst = sc.render_raycams_tensor(cams, W, H, format=fmt, **kw)
            got, ticket = sc.enqueue_render_raycams_tensor(cams, W, H, format=fmt, **kw)
            est = sc.enqueue_stats(ticket)
            torch.cuda.synchronize()
            assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes(), (kw.get("max_level"), fmt)
            assert all(est[k] == rst[k] for k in STAT_KEYS), (est, rst)
    # with geometry planes
    ref, rst, rplanes = sc.render_raycams_tensor(cams, W, H, aovs=AOVS, max_level=2)
    got, ticket, planes = sc.enqueue_render_raycams_tensor(cams, W, H, aovs=AOVS, max_level=2)
    est = sc.enqueue_stats(ticket)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes() and all(est[k] == rst[k] for k in STAT_KEYS)
    for k in AOVS:
        assert planes[k].cpu().numpy().tobytes() == rplanes[k].cpu().numpy().tobytes(), k
    # ordered behind the work the caller put on the stream before it
    s = torch.cuda.Stream()
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device="cuda")
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            big = big @ big  # keeps the stream busy
        out.fill_(-7.0)  # enqueued BEFORE the call: the frames must land after it
    table = pkg.raycam_array(cams)
    _, ticket = sc.enqueue_render_raycams_tensor(table, W, H, out=out, stream=s, max_level=2)
    table[:] = 0.0  # (the cameras are reusable at once)
    with torch.cuda.stream(s):
        copy = out.clone()  # enqueued AFTER the call: sees the frames
    torch.cuda.synchronize()
    assert copy.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes() and out.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()
    assert all(sc.enqueue_stats(ticket)[k] == rst[k] for k in STAT_KEYS)
    # trace: the table of an asynchronous call may be overwritten at once, too
    want, _ = _trace(pkg, sc, cams, 64, 48)
    hb, hi, hok = _guarded(B * 64 * 48 * 16)
    table = pkg.raycam_array(cams)
    with torch.cuda.stream(s):
        big = torch.randn(4096, 4096, device="cuda")
        for _ in range(8):
            big = big @ big
    sc.trace_raycams_device(table, 64, 48, hi.data_ptr(), stream=s.cuda_stream)
    table[:] = 0.0
    assert hok() and hi.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("name", ["cornell", "dragon"])
def test_light_sets_form(pkg, world, name):
    sd, sc, _ = world(name)
    W, H = SIZES[0]
    cams = _cams(pkg, name, W, H)[:5]
    base = np.asarray(sd.point_lights, np.float32).reshape(-1, 6)
    moved = base.copy()
    moved[:, 0:3] += np.float32([0.3, -0.2, 0.1])
    moved[:, 3:6] *= np.float32(0.5)
    sets = [base, moved, np.concatenate([base, moved]), np.zeros((0, 6), np.float32)]
    for depth in (1, 2, 4):
        for fmt in FORMATS:
            t, st = sc.render_raycams_tensor(cams, W, H, format=fmt, light_sets=sets, max_level=depth)
            torch.cuda.synchronize()
            a = t.cpu().numpy()
            assert a.shape[:2] == (len(cams), len(sets))
            for s, lights in enumerate(sets):
                single, _ = sc.render_raycams_tensor(cams, W, H, format=fmt, lights=lights, max_level=depth)
                torch.cuda.synchronize()
                single = single.cpu().numpy()
                for b in range(len(cams)):
                    assert a[b, s].tobytes() == single[b].tobytes(), (name, depth, fmt, b, s)
            assert st["primary_rays"] == len(cams) * W * H
    # spherical sets: frame (b, s) is the single render under set s's lights, the draws keyed by the in-view pixel and the index in the set
    if name == "cornell":
        sph = pkg.scenes.CORNELL_SPHERICAL_LIGHTS.copy()
        soft = dict(units=pkg.unit_vector_table(1000, 5), samples=4, seed=3)
        sph_sets = [sph, sph[:1], np.zeros((0, 7), np.float32), sph[::-1].copy()]
        t, _ = sc.render_raycams_tensor(cams, W, H, light_sets=sets, spherical_sets=sph_sets, max_level=2, **soft)
        torch.cuda.synchronize()
        a = t.cpu().numpy()
        for s in range(len(sets)):
            kw = dict(spherical=sph_sets[s], **soft) if len(sph_sets[s]) else {}
            single, _ = sc.render_raycams_tensor(cams, W, H, lights=sets[s], max_level=2, **kw)
            torch.cuda.synchronize()
            assert a[:, s].tobytes() == single.cpu().numpy().tobytes(), s


def test_existing_state_is_left_alone(pkg, scene_data):
    sc = pkg.Scene(scene_data("cornell"))
    W, H = 96, 64
    cam = pkg.scenes.default_camera(W, H)
    first, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == EXACT
    for _ in range(2):
        rgb, _ = sc.render(cam, W, H, max_level=2)
        assert sc.last_render_path() == PREDICTED and rgb.tobytes() == first.tobytes()
    t0, _ = sc.render_tensor(cam, W, H, format="rgba8", max_level=2)
    torch.cuda.synchronize()
    t0 = t0.cpu().numpy()
    # ray-camera batches of the same and of other shapes and depths in between, blocking, enqueued, light sets, traces
    cams = _cams(pkg, "cornell", W, H)
    sc.render_raycams_tensor(cams, W, H, max_level=2)
    sc.render_raycams_tensor(cams[:2], 33, 17, format="chw", max_level=4)
    sc.render_raycams_tensor(pkg.RayCamera.from_trackball(cam, W, H), W, H, max_level=2)
    _, ticket = sc.enqueue_render_raycams_tensor(cams, W, H, max_level=2)
    sc.enqueue_stats(ticket)
    sc.render_raycams_tensor(cams[:3], W, H, light_sets=[np.asarray(sc.sd.point_lights, np.float32).reshape(-1, 6)] * 2, max_level=2)
    _trace(pkg, sc, cams, W, H)
    rgb, _ = sc.render(cam, W, H, max_level=2)
    assert sc.last_render_path() == PREDICTED, "a ray-camera batch must not touch the scene's prediction record"
    assert rgb.tobytes() == first.tobytes()
    t1, _ = sc.render_tensor(cam, W, H, format="rgba8", max_level=2)
    torch.cuda.synchronize()
    assert sc.last_render_path() == PREDICTED and t1.cpu().numpy().tobytes() == t0.tobytes()
    sc.close()


def test_frame_hints_are_left_alone(pkg):
    pkg.debug_set_hint_thresholds(100, 60)  # (most tiles that reach the tree are hard: the hint lists are busy)
    pkg.set_frame_hints(1)
    try:
        sc = pkg.Scene(pkg.scenes.make_dragon(60_000))
        W, H = 320, 200
        cam = pkg.scenes.default_camera(W, H)

        def single():
            h = torch.full((W * H * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
            sc.trace_primary_device(cam, W, H, h.data_ptr())
            torch.cuda.synchronize()
            return h.cpu().numpy().tobytes()

        h0 = single()
        for _ in range(4):  # hinted frames
            assert single() == h0
        counts = sc.hint_counts()
        cams = _cams(pkg, "dragon", W, H)
        _trace(pkg, sc, cams[:3], W, H)
        sc.render_raycams_tensor(cams[:2], W, H, max_level=2)
        assert sc.hint_counts() == counts, "a ray-camera batch must not touch the frame hints"
        for _ in range(4):
            assert single() == h0
        sc.close()
    finally:
        pkg.set_frame_hints(-1)
        pkg.debug_set_hint_thresholds(0, 0)


def test_from_trackball_frames_are_close_to_the_trackball(pkg, world):
    """Not part of the contract's exactness: the fitted camera's primary hits agree with the Trackball's on >= 99.5 % of the pixels."""
    for name in ("cornell", "dragon"):
        sd, sc, _ = world(name)
        W, H = 96, 64
        cam = pkg.scenes.default_camera(W, H)
        hits, _ = _trace(pkg, sc, [pkg.RayCamera.from_trackball(cam, W, H)], W, H)
        h = torch.zeros((W * H * 16,), dtype=torch.uint8, device="cuda")
        sc.trace_primary_device(cam, W, H, h.data_ptr())
        torch.cuda.synchronize()
        ref = h.cpu().numpy().view(pkg.HIT_DTYPE)
        assert float((hits[0]["hit"] == ref["hit"]).mean()) >= 0.995 and float(ref["hit"].mean()) >= 0.05

"""GPU tests of the surface attributes (include/cgrt.h cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_*_device; Scene.
hit_barycentrics / interpolate_hits and their *_device / *_tensor forms, surface_views_tensor, surface_raycams_tensor).

Everything is bit for bit (conftest.same_bits): the device's weights are those of tests/surface_ref.py, the numpy restatement of
ray_tracing.cpp:13-21 and :94-97 that tests/test_surface_cpu.py holds to the CPU oracle; an interpolated attribute is the numpy mix of
those weights; with the vertex normals as the attribute, normalised and flipped, it is the normal the library's own trace wrote.  The
frame forms equal the list forms on the frame's generated rays.  Every device output lies between guards of sentinel bytes."""
import dataclasses
import threading

import numpy as np
import pytest

import surface_ref as sr
from conftest import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
FLT_MAX = np.finfo(np.float32).max
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")


class Guarded:
    """nbytes of device memory between two guards, all of it sentinel bytes before the call."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def tensor(self, shape):
        return self.buf[PAD : PAD + self.n].view(torch.float32).view(tuple(shape))

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n :] == SENTINEL).all())


def _out(shape):
    g = Guarded(4 * int(np.prod(shape, dtype=np.int64)))
    return g, g.tensor(shape)


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _dev_rays(rays):
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 7).copy()).cuda()


def _dev_hits(hits):
    return torch.from_numpy(np.ascontiguousarray(hits).view(np.int32).reshape(-1, 4).copy()).cuda()


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(same_bits(a, b).all())


@pytest.fixture(scope="module")
def mixed(pkg, scene_data):
    """The blob with two spheres beside it: triangle hits, sphere hits and misses in one list or frame."""
    sd = scene_data("blob")
    hi = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3].max(0)
    sph = np.asarray([[hi[0], hi[1], 0.0, 0.45 * hi[0], -1], [-hi[0], 0.0, hi[2], 0.4 * hi[0], 0]], np.float32)
    sd = dataclasses.replace(sd, spheres=sph, name="blob+spheres")
    sc = pkg.Scene(sd, device=0)
    yield sd, sc
    sc.close()


@pytest.fixture(scope="module")
def mixed_rays(pkg, mixed):
    sd, sc = mixed
    rays = sr.random_rays(sd, 4097, 23)
    hits, _ = sc.intersect(rays)
    first = np.flatnonzero(sr.triangle_mask(sd, hits["hit"], hits["prim_id"]))[0]
    rays[[0, first]] = rays[[first, 0]]  # n = 1: a triangle hit
    return rays


def _classes(sd, hits):
    tri = sr.triangle_mask(sd, hits["hit"], hits["prim_id"])
    return int(tri.sum()), int(((hits["hit"] != 0) & ~tri).sum()), int((hits["hit"] == 0).sum())


# ---- 1. barycentrics of ray lists ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_barycentrics_equal_the_restatement(pkg, mixed, mixed_rays, n):
    sd, sc = mixed
    rays = mixed_rays[:n]
    results = []
    try:
        for shape in (0, 1, 2, 3):
            pkg.set_kernel_shape(shape)
            hits, _ = sc.intersect(rays)
            results.append(hits)
            ntri, nsph, nmiss = _classes(sd, hits)
            assert ntri >= 1 and (n < 63 or (nsph >= 1 and nmiss >= 1)), (n, ntri, nsph, nmiss)
            ref = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
            host = sc.hit_barycentrics(rays, hits)
            assert _same(host, ref), (n, shape, "host form")
            g, out = _out((n, 3))
            got = sc.hit_barycentrics_tensor(_dev_rays(rays), _dev_hits(hits), out=out)
            assert got is out and _same(_np(out), ref), (n, shape, "device form")
            assert g.intact()
            assert not ref[~sr.triangle_mask(sd, hits["hit"], hits["prim_id"])].any(), "zeros where the definition says zeros"
    finally:
        pkg.set_kernel_shape(-1)
    for h in results[1:]:
        assert h.tobytes() == results[0].tobytes(), "the hits themselves do not depend on the kernel shape"


# ---- 2. tie to the normal the library already writes ----
@pytest.mark.parametrize("name", ["triangle", "cube", "cornell", "monkey", "blob"])
def test_vertex_normals_interpolate_to_the_traced_normal(pkg, orc, scene_data, name):
    sd = scene_data(name)
    sc = pkg.Scene(sd, device=0)
    try:
        rays = np.concatenate([orc.generate_rays(pkg.scenes.default_camera(64, 48), 64, 48), sr.random_rays(sd, 2000, 3)])
        n = len(rays)
        d_rays = _dev_rays(rays)
        d_hits = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        d_nrm = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        sc.intersect_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_nrm.data_ptr())
        vn = torch.from_numpy(np.ascontiguousarray(np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 3:6])).cuda()
        g, out = _out((n, 3))
        sc.interpolate_hits_tensor(d_rays, d_hits, vn, out=out)
        mixed_n, hits, traced = _np(out), _np(d_hits).view(pkg.HIT_DTYPE).reshape(-1), _np(d_nrm)
        assert g.intact()
        m = sr.triangle_mask(sd, hits["hit"], hits["prim_id"])
        assert m.sum() >= (1 if name == "triangle" else 500), (name, int(m.sum()))
        mine = sr.finish_normal(mixed_n[m], sr.facing(sd, rays[m], hits["prim_id"][m]))
        bad = ~same_bits(mine, traced[m]).all(1)
        assert not bad.any(), (name, int(bad.sum()), mine[bad][:2], traced[m][bad][:2])
        assert _same(sc.interpolate_hits(rays, hits, _np(vn)), mixed_n), "host form"
    finally:
        sc.close()


# ---- 3. channel counts ----
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 16, 33, 256])
def test_channel_counts(pkg, mixed, mixed_rays, C):
    sd, sc = mixed
    n = 1000 if C < 256 else 200
    rays = mixed_rays[:n]
    hits, _ = sc.intersect(rays)
    nverts = len(sd.pos_nrm)
    attr = np.random.default_rng(100 + C).standard_normal((nverts, C)).astype(np.float32)
    ref = sr.mix(sd, sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"]), hits["prim_id"], hits["hit"], attr)
    d_rays, d_hits = _dev_rays(rays), _dev_hits(hits)
    g, out = _out((n, C))
    sc.interpolate_hits_tensor(d_rays, d_hits, torch.from_numpy(attr).cuda(), out=out)
    assert _same(_np(out), ref), (C, "a table of its own")
    assert g.intact()
    # the table as a view into a larger allocation, 4 bytes off a 16-byte boundary (no 16-byte loads there), into a new tensor
    big = torch.full((nverts * C + 64,), float("nan"), dtype=torch.float32, device="cuda")
    off = 1 + (-(big.data_ptr() // 4) % 4)
    view = big[off : off + nverts * C].view(nverts, C)
    view.copy_(torch.from_numpy(attr))
    assert view.data_ptr() % 16 == 4
    assert _same(_np(sc.interpolate_hits_tensor(d_rays, d_hits, view)), ref), (C, "a view into a larger allocation")
    assert _same(sc.interpolate_hits(rays, hits, attr), ref), (C, "host form")
    assert not ref[~sr.triangle_mask(sd, hits["hit"], hits["prim_id"])].any()


# ---- 4. frames ----
def _moved(pkg, W, H, i):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[3] += np.float32(0.3 * i)
    cam[4] += np.float32(0.5 * i)
    return cam


def _plane_hits(pkg, depth, prim):
    h = np.zeros(depth.size, pkg.HIT_DTYPE)
    h["t"], h["prim_id"] = depth.reshape(-1), prim.reshape(-1).view(np.uint32)
    h["hit"] = h["prim_id"] != pkg.NO_PRIM
    h["material_id"] = -1
    return h


def _hwc(a, chw):
    return np.moveaxis(a, -3, -1) if chw else a


def _check_frames(pkg, sd, sc, surface, cams, rays, W, H, depth, prim, chw, what):
    """surface(cams, W, H, depth, prim_id, ...) against the list forms on `rays` (B * H * W, view after view) and the planes' hits."""
    B = len(rays) // (W * H)
    hits = _plane_hits(pkg, _np(depth), _np(prim))
    ntri, nsph, nmiss = _classes(sd, hits)
    assert ntri > 0 and nmiss + nsph > 0, (what, ntri, nsph, nmiss)
    nverts = len(sd.pos_nrm)
    for C in (5, 8):
        attr = np.random.default_rng(C).standard_normal((nverts, C)).astype(np.float32)
        ref_b = sc.hit_barycentrics(rays, hits).reshape(B, H, W, 3)
        ref_a = sc.interpolate_hits(rays, hits, attr).reshape(B, H, W, C)
        d_attr = torch.from_numpy(attr).cuda()
        sb, sa = ((B, 3, H, W), (B, C, H, W)) if chw else ((B, H, W, 3), (B, H, W, C))
        for want_bary, want_attr in ((True, False), (False, True), (True, True)):
            gb, ob = _out(sb)
            ga, oa = _out(sa)
            out = ({"bary": ob} if want_bary else {}) | ({"attr": oa} if want_attr else {})
            res = surface(cams, W, H, depth, prim, attr=d_attr if want_attr else None, want_bary=want_bary, chw=chw, out=out)
            assert set(res) == set(out), (what, set(res))
            if want_bary:
                assert _same(_hwc(_np(res["bary"]), chw), ref_b), (what, C, "bary", want_attr)
            if want_attr:
                assert _same(_hwc(_np(res["attr"]), chw), ref_a), (what, C, "attr", want_bary)
            assert gb.intact() and ga.intact(), (what, "guards")
            if not want_bary:
                assert bool((gb.buf == SENTINEL).all()), "an output that was not requested is not touched"
    return nsph


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 17), (72, 40)])
def test_trackball_frames_equal_the_list_form(pkg, mixed, W, H, B, chw):
    sd, sc = mixed
    cams = np.stack([_moved(pkg, W, H, i) for i in range(B)])
    _, _, planes = sc.render_views_aov_tensor(cams, W, H, aovs=("depth", "prim_id"))
    rays = np.concatenate([sc.generate_rays(c, W, H) for c in cams])
    _check_frames(pkg, sd, sc, sc.surface_views_tensor, cams, rays, W, H, planes["depth"], planes["prim_id"], chw, ("trackball", W, H, B, chw))


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 17), (72, 40)])
def test_raycam_frames_equal_the_list_form(pkg, mixed, W, H, B, chw):
    sd, sc = mixed
    # the last camera is a tile of a frame twice the size, the others whole W x H frames
    cams = [pkg.RayCamera.from_trackball(_moved(pkg, W, H, i), W, H) for i in range(B - 1)]
    cams.append(pkg.RayCamera.from_trackball(_moved(pkg, 2 * W, 2 * H, B - 1), 2 * W, 2 * H).tile(W // 2, H // 3))
    _, _, planes = sc.render_raycams_tensor(cams, W, H, aovs=("depth", "prim_id"))
    rays = np.concatenate([sc.generate_rays_raycam(c, W, H) for c in cams])
    _check_frames(pkg, sd, sc, sc.surface_raycams_tensor, cams, rays, W, H, planes["depth"], planes["prim_id"], chw, ("raycam", W, H, B, chw))


def test_single_camera_and_anti_aliased_planes(pkg, mixed):
    sd, sc = mixed
    W, H = 33, 17
    cam = _moved(pkg, W, H, 1)
    _, _, planes = sc.render_aov_tensor(cam, W, H, aovs=("depth", "prim_id"), aa=True)
    assert tuple(planes["depth"].shape) == (2 * H, 2 * W)
    rays = sc.generate_rays(cam, 2 * W, 2 * H)  # finding AA3: the sub-sample rays are the 2W x 2H frame's
    hits = _plane_hits(pkg, _np(planes["depth"]), _np(planes["prim_id"]))
    res = sc.surface_views_tensor(cam, 2 * W, 2 * H, planes["depth"], planes["prim_id"])  # one camera, (H, W) planes
    assert tuple(res["bary"].shape) == (2 * H, 2 * W, 3)
    assert _same(_np(res["bary"]).reshape(-1, 3), sc.hit_barycentrics(rays, hits))
    assert _same(_np(res["bary"]).reshape(-1, 3), sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"]))
    with pytest.raises(ValueError):
        sc.surface_views_tensor(cam, 2 * W, 2 * H, planes["depth"], planes["prim_id"], want_bary=False)
    with pytest.raises(ValueError):
        sc.surface_views_tensor(cam, W, H, planes["depth"], planes["prim_id"])


# ---- 5. robustness, without provoking anything ----
def test_out_of_range_ids_and_odd_parameters(pkg, mixed, mixed_rays):
    sd, sc = mixed
    rays = mixed_rays[:64].copy()
    hits, _ = sc.intersect(rays)
    tri = np.flatnonzero(sr.triangle_mask(sd, hits["hit"], hits["prim_id"]))
    assert len(tri) >= 8
    hits["hit"][tri[:6]] = 1
    for k, prim in enumerate((sd.ntris, sd.ntris + len(sd.spheres), 0xFFFFFFFE, pkg.NO_PRIM)):
        hits["prim_id"][tri[k]] = prim
    hits["t"][tri[4]] = np.nan
    hits["t"][tri[5]] = FLT_MAX
    hits["hit"][tri[6]] = 0  # a valid id that is not a hit
    nverts = len(sd.pos_nrm)
    attr = np.random.default_rng(1).standard_normal((nverts, 4)).astype(np.float32)
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    assert not w[tri[:4]].any() and not w[tri[6]].any() and np.isnan(w[tri[4]]).all()
    gb, ob = _out((64, 3))
    ga, oa = _out((64, 4))
    sc.hit_barycentrics_tensor(_dev_rays(rays), _dev_hits(hits), out=ob)
    sc.interpolate_hits_tensor(_dev_rays(rays), _dev_hits(hits), torch.from_numpy(attr).cuda(), out=oa)
    assert _same(_np(ob), w) and _same(_np(oa), sr.mix(sd, w, hits["prim_id"], hits["hit"], attr))
    assert gb.intact() and ga.intact()
    assert (_np(ob)[tri[:4]].view(np.uint32) == 0).all() and (_np(oa)[tri[:4]].view(np.uint32) == 0).all(), "+0.0, whatever the table holds"


def test_zero_area_triangle_gives_what_the_formula_gives(pkg):
    pn = np.zeros((6, 6), np.float32)
    pn[:, 5] = 1
    pn[0:3, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    pn[3:6, 0:3] = [[0, 0, 1], [1, 1, 1], [2, 2, 1]]  # collinear: zero area
    sd = pkg.scenes.SceneData(pos_nrm=pn, tri=np.asarray([[0, 1, 2], [3, 4, 5]], np.uint32), tri_mesh=np.zeros(2, np.uint32),
                              materials=np.asarray([[0.5, 0.5, 0.5, 0, 0, 0, 1, 1]], np.float32))
    sc = pkg.Scene(sd, device=0)
    try:
        rays = np.asarray([[0.25, 0.25, 2, 0, 0, -1, FLT_MAX], [0.5, 0.5, 2, 0, 0, -1, FLT_MAX]], np.float32)
        hits = np.zeros(2, pkg.HIT_DTYPE)
        hits["t"], hits["prim_id"], hits["hit"] = [2.0, 1.0], [0, 1], 1
        ref = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
        assert _same(ref[0], [0.5, 0.25, 0.25]) and not np.isfinite(ref[1]).any()
        g, out = _out((2, 3))
        sc.hit_barycentrics_tensor(_dev_rays(rays), _dev_hits(hits), out=out)
        assert _same(_np(out), ref) and g.intact()
        assert _same(sc.hit_barycentrics(rays, hits), ref)
    finally:
        sc.close()


# ---- 6. nothing else moves ----
def test_nothing_else_moves(pkg, scene_data):
    sd = scene_data("cornell")
    a, b = pkg.Scene(sd, device=0), pkg.Scene(sd, device=0)
    try:
        assert a.device_bytes() == b.device_bytes() and a.layout_hash() == b.layout_hash()
        W, H = 64, 48
        cam = pkg.scenes.default_camera(W, H)
        for _ in range(3):
            before = a.render(cam, W, H)
        path = a.last_render_path()
        rays = sr.random_rays(sd, 500, 9)
        hits, _ = a.intersect(rays)
        a.hit_barycentrics(rays, hits)
        a.interpolate_hits(rays, hits, np.ones((len(sd.pos_nrm), 7), np.float32))
        _, _, planes = a.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
        a.surface_views_tensor(cam, W, H, planes["depth"], planes["prim_id"])
        torch.cuda.synchronize()
        ref = b.render(cam, W, H)
        for _ in range(2):
            ref = b.render(cam, W, H)
        b.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash()
        assert a.device_bytes() == b.device_bytes() + 16 * sd.ntris, "the lookup table, 16 bytes per triangle, and nothing else"
    finally:
        a.close()
        b.close()


# ---- 7. streams and threads ----
def test_streams_and_threads(pkg, mixed, mixed_rays):
    sd, sc = mixed
    nverts = len(sd.pos_nrm)
    attr = torch.from_numpy(np.random.default_rng(2).standard_normal((nverts, 6)).astype(np.float32)).cuda()
    jobs = []
    for k in range(8):
        rays = mixed_rays[100 * k : 100 * k + 37 + 11 * k]
        hits, _ = sc.intersect(rays)
        jobs.append((_dev_rays(rays), _dev_hits(hits)))
    serial = [(_np(sc.hit_barycentrics_tensor(r, h)), _np(sc.interpolate_hits_tensor(r, h, attr))) for r, h in jobs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got, errors = {}, []

    def work(tid):
        try:
            for it in range(6):
                for k in range(tid, len(jobs), 4):
                    s = streams[(tid + it + k) % 2]
                    r, h = jobs[k]
                    got[(tid, it, k)] = (sc.hit_barycentrics_tensor(r, h, stream=s), sc.interpolate_hits_tensor(r, h, attr, stream=s), s)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    assert len(got) == 6 * len(jobs)
    for (tid, it, k), (b, a, _) in got.items():
        assert _same(b.cpu().numpy(), serial[k][0]) and _same(a.cpu().numpy(), serial[k][1]), (tid, it, k)

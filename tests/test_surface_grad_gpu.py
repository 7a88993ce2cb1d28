"""GPU tests of the gradients of the surface attributes back to the per-vertex table (include/cgrt.h cgrt_interpolate_hits_grad*,
cgrt_surface_*_grad_device; Scene.interpolate_hits_grad and its *_device / *_tensor forms, surface_views_grad_tensor,
surface_raycams_grad_tensor, and the autograd path of the three forward tensor entries).

The order of the additions into one element is unspecified, so three kinds of check:
  * bit for bit where every order gives the same bits: the unit square with weights in sixteenths (thirty-seconds for its frame) and
    small integer gradients (section 1), and single contributions into a zeroed table (section 2);
  * the derived bound of tests/surface_grad_ref.py against its float64 restatement everywhere else (elements with more than 512
    contributions are counted, never compared; the inputs keep them away);
  * bytes that must not move: rows no valid item names, the memory around the table, everything else a scene owns."""
import dataclasses
import threading

import numpy as np
import pytest

import surface_grad_ref as gr
import surface_ref as sr
from conftest import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
FLT_MAX = np.finfo(np.float32).max
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")
MAPS = (None, "element", "item", "item_plain")  # CGRT_SURFACE_GRAD_MAP: the shipped policy, and each mapping forced


class Guarded:
    """A float32 tensor of `shape` in device memory between two guards of sentinel bytes."""

    def __init__(self, shape):
        self.n = 4 * int(np.prod(shape, dtype=np.int64))
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.t = self.buf[PAD : PAD + self.n].view(torch.float32).view(tuple(shape))

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n :] == SENTINEL).all())


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_rays(rays):
    return _dev(np.ascontiguousarray(rays).view(np.float32).reshape(-1, 7).copy())


def _dev_hits(hits):
    return _dev(np.ascontiguousarray(hits).view(np.int32).reshape(-1, 4).copy())


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _nverts(sd):
    return len(np.asarray(sd.pos_nrm).reshape(-1, 6))


def _hits(pkg, t, prim, hit=1):
    h = np.zeros(len(prim), pkg.HIT_DTYPE)
    h["t"], h["prim_id"], h["hit"], h["material_id"] = t, np.asarray(prim, np.uint32), hit, -1
    return h


def _values(rng, shape):
    """float32 with |x| in [2^-10, 2^10], either sign."""
    return (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** rng.uniform(-10, 10, shape)).astype(np.float32)


# ---- 1. exact under contention: the unit square ----
PTS = np.asarray([(a, b) for a in range(1, 16) for b in range(1, 16) if a + b != 16], np.int64)
PTS_PRIM = (PTS.sum(1) > 16).astype(np.uint32)
assert len(PTS) == 210


@pytest.fixture(scope="module")
def square(pkg):
    """The unit square as two right triangles, and the barycentrics of the 210 points: sixteenths, on the host and on the device."""
    pn = np.zeros((4, 6), np.float32)
    pn[:, 5] = 1
    pn[:, 0:3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    sd = pkg.scenes.SceneData(pos_nrm=pn, tri=np.asarray([[0, 1, 2], [1, 3, 2]], np.uint32), tri_mesh=np.zeros(2, np.uint32),
                              materials=np.asarray([[0.5, 0.5, 0.5, 0, 0, 0, 1, 1]], np.float32))
    sc = pkg.Scene(sd, device=0)
    rays, hits = _square_list(pkg, np.arange(len(PTS)))
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    assert (w * 16 == np.round(w * 16)).all() and w.min() >= 1 / 16 and w.max() <= 14 / 16, "the precondition of the exactness argument"
    assert _bits_equal(_np(sc.hit_barycentrics_tensor(_dev_rays(rays), _dev_hits(hits))), w), "the device's weights are these very values"
    yield sd, sc
    sc.close()


def _square_list(pkg, idx):
    p = PTS[idx]
    rays = np.zeros((len(p), 7), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 5], rays[:, 6] = p[:, 0] / 16.0, p[:, 1] / 16.0, 1.0, -1.0, FLT_MAX
    return rays, _hits(pkg, 1.0, PTS_PRIM[idx])


def _order(kind, n, rng):
    on = [np.flatnonzero(PTS_PRIM == k) for k in (0, 1)]
    if kind == "one_triangle":
        return on[0][(7 * np.arange(n)) % len(on[0])]
    if kind == "shuffled":
        return rng.integers(0, len(PTS), n)
    idx, k = [], 0  # runs of one prim_id, lengths 1, 2, 3, 5, 64, 70 in turn: they straddle the waves' boundaries
    while sum(map(len, idx)) < n:
        idx.append(rng.choice(on[k % 2], (1, 2, 3, 5, 64, 70)[k % 6]))
        k += 1
    return np.concatenate(idx)[:n]


def _exact(sd, rays, hits, g, init):
    """The one value every order of the additions gives, when every product and partial sum is exact."""
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    ref, _, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()
    return ref.astype(np.float32), m


@pytest.mark.parametrize("C", [1, 3, 4, 5, 32, 256])
@pytest.mark.parametrize("kind", ["one_triangle", "runs", "shuffled"])
def test_exact_under_contention_lists(pkg, square, monkeypatch, kind, C):
    sd, sc = square
    rng = np.random.default_rng(1000 + C)
    for n in (1, 63, 64, 65, 320, 4097):
        if C == 256 and n > 320:
            continue
        rays, hits = _square_list(pkg, _order(kind, n, rng))
        g = rng.integers(-8, 9, (n, C)).astype(np.float32)
        d_rays, d_hits, d_g = _dev_rays(rays), _dev_hits(hits), _dev(g)
        for init in (np.zeros((4, C), np.float32), rng.integers(-8, 9, (4, C)).astype(np.float32)):
            want, _ = _exact(sd, rays, hits, g, init)
            for mapping in MAPS:
                if mapping is None:
                    monkeypatch.delenv("CGRT_SURFACE_GRAD_MAP", raising=False)
                else:
                    monkeypatch.setenv("CGRT_SURFACE_GRAD_MAP", mapping)
                table = Guarded((4, C))
                table.t.copy_(_dev(init))
                got = sc.interpolate_hits_grad_tensor(d_rays, d_hits, d_g, grad_attr=table.t)
                assert got is table.t and _bits_equal(_np(got), want), (kind, C, n, mapping, bool(init.any()))
                assert table.intact()
            monkeypatch.delenv("CGRT_SURFACE_GRAD_MAP", raising=False)
            if n == 65:
                host = sc.interpolate_hits_grad(rays, hits, g, grad_attr=init.copy())
                assert _bits_equal(host, want), (kind, C, "host form")
    if C == 3:
        assert _bits_equal(sc.interpolate_hits_grad(rays, hits, g), _exact(sd, rays, hits, g, None)[0]), "host form, a new table"


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
def test_exact_under_contention_frames(pkg, square, monkeypatch, B, chw):
    sd, sc = square
    W = H = 16
    cam = pkg.RayCamera.from_fields((1 / 32, 1 / 32, 1), (1 / 16, 0, 0), (0, 1 / 16, 0), (0, 0, -1), (0, 0, 0), (0, 0, 0))
    y, x = np.mgrid[0:H, 0:W]
    prim = np.where(x + y < 15, 0, np.where(x + y == 15, pkg.NO_PRIM, 1)).astype(np.uint32)  # (the diagonal's pixels: misses)
    rays = np.concatenate([sc.generate_rays_raycam(cam, W, H)] * B)
    hits = _hits(pkg, 1.0, np.tile(prim.reshape(-1), B))
    hits["hit"] = hits["prim_id"] != pkg.NO_PRIM
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    ok = hits["hit"] != 0
    assert (w * 32 == np.round(w * 32)).all() and w[ok].min() >= 1 / 32 and ok.sum() == B * 240
    d_depth = torch.ones((B, H, W), dtype=torch.float32, device="cuda")
    d_prim = _dev(np.tile(prim.view(np.int32), (B, 1, 1)))
    bary = sc.surface_raycams_tensor([cam] * B, W, H, d_depth, d_prim)["bary"]
    assert _bits_equal(_np(bary).reshape(-1, 3), w), "the device's weights are these very values"
    rng = np.random.default_rng(77 + B)
    for C in (1, 5, 32):
        g = rng.integers(-8, 9, (B * H * W, C)).astype(np.float32)
        g_dev = g.reshape(B, H, W, C)
        d_g = _dev(np.moveaxis(g_dev, -1, 1) if chw else g_dev)
        for init in (np.zeros((4, C), np.float32), rng.integers(-8, 9, (4, C)).astype(np.float32)):
            want, _ = _exact(sd, rays, hits, g, init)
            for mapping in MAPS:
                if mapping is None:
                    monkeypatch.delenv("CGRT_SURFACE_GRAD_MAP", raising=False)
                else:
                    monkeypatch.setenv("CGRT_SURFACE_GRAD_MAP", mapping)
                table = Guarded((4, C))
                table.t.copy_(_dev(init))
                got = sc.surface_raycams_grad_tensor([cam] * B, W, H, d_depth, d_prim, d_g, chw=chw, grad_attr=table.t)
                assert got is table.t and _bits_equal(_np(got), want), (B, chw, C, mapping, bool(init.any()))
                assert table.intact()
    monkeypatch.delenv("CGRT_SURFACE_GRAD_MAP", raising=False)


# ---- 2. single contributions are the rounded products ----
@pytest.fixture(scope="module")
def soup(pkg):
    """257 triangles that share no vertex, the rows of their corners shuffled over the table, and one interior ray each."""
    rng = np.random.default_rng(5)
    T = 257
    cell = rng.uniform(0.3, 0.7, (T, 3, 2))
    cell[:, 1, 0] += 1.0  # (never degenerate: the edge vectors are (1 + dx, dy) and (dx', 1 + dy') with |d| <= 0.4)
    cell[:, 2, 1] += 1.0
    pos = np.zeros((T, 3, 3), np.float32)
    pos[:, :, 0:2] = cell + 3.0 * np.arange(T)[:, None, None] * np.asarray([1.0, 0.0])
    rows = rng.permutation(3 * T).reshape(T, 3)
    pn = np.zeros((3 * T, 6), np.float32)
    pn[:, 5] = 1
    pn[rows.reshape(-1), 0:3] = pos.reshape(-1, 3)
    sd = pkg.scenes.SceneData(pos_nrm=pn, tri=rows.astype(np.uint32), tri_mesh=np.zeros(T, np.uint32),
                              materials=np.asarray([[0.5, 0.5, 0.5, 0, 0, 0, 1, 1]], np.float32))
    b = rng.dirichlet((2.0, 2.0, 2.0), T)
    p = (b[:, :, None] * pos.astype(np.float64)).sum(1)
    rays = np.zeros((T, 7), np.float32)
    rays[:, 0:2], rays[:, 2], rays[:, 5], rays[:, 6] = p[:, 0:2], 1.0, -1.0, FLT_MAX
    sc = pkg.Scene(sd, device=0)
    yield sd, sc, rays, _hits(pkg, 1.0, np.arange(T))
    sc.close()


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 16, 33, 256])
def test_single_contributions_are_the_rounded_products(pkg, soup, C):
    sd, sc, rays, hits = soup
    rng = np.random.default_rng(C)
    for n in (1, 63, 64, 65, 257):
        d_rays, d_hits = _dev_rays(rays[:n]), _dev_hits(hits[:n])
        bary = _np(sc.hit_barycentrics_tensor(d_rays, d_hits))
        assert (bary > 0).all()
        g = _values(rng, (n, C))
        table = Guarded((_nverts(sd), C))
        table.t.zero_()
        sc.interpolate_hits_grad_tensor(d_rays, d_hits, _dev(g), grad_attr=table.t)
        want = np.zeros((_nverts(sd), C), np.float32)
        tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)[:n]
        for k in range(3):
            want[tri[:, k]] = bary[:, k : k + 1] * g  # float32 products, each rounded once
        assert _bits_equal(_np(table.t), want), (C, n)
        assert table.intact()


# ---- 3. real scenes to the bound ----
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


def _capped_list(pkg, sd, sc, n, seed):
    """n seeded rays and their hits, with out-of-range ids written into some of them, and hits turned into misses wherever a vertex
    would otherwise collect more than M_CAP contributions: the restatement alone stays under the cap."""
    rays = sr.random_rays(sd, n, seed)
    hits, _ = sc.intersect(rays)
    hits = hits.copy()
    tri_hits = np.flatnonzero(sr.triangle_mask(sd, hits["hit"], hits["prim_id"]))
    for k, prim in enumerate((sd.ntris, sd.ntris + len(sd.spheres), 0xFFFFFFFE, pkg.NO_PRIM)):
        hits["prim_id"][tri_hits[5 * k + 3]] = prim
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    count = np.zeros(_nverts(sd), np.int64)
    for i in np.flatnonzero(sr.triangle_mask(sd, hits["hit"], hits["prim_id"])):
        v = tri[hits["prim_id"][i]]
        if (count[v] >= gr.M_CAP - 2).any():
            hits["hit"][i] = 0
        else:
            np.add.at(count, v, 1)
    return rays, hits


@pytest.mark.parametrize("C", [3, 32])
@pytest.mark.parametrize("name", ["mixed", "monkey", "cornell"])
def test_real_scenes_to_the_bound(pkg, scene_data, mixed, name, C):
    sd, sc = mixed if name == "mixed" else (scene_data(name), None)
    own = sc is None
    if own:
        sc = pkg.Scene(sd, device=0)
    try:
        n = 4097
        rays, hits = _capped_list(pkg, sd, sc, n, 31)
        ok = sr.triangle_mask(sd, hits["hit"], hits["prim_id"])
        assert ok.sum() >= 300 and (~ok).sum() >= 20, (name, int(ok.sum()))
        if name == "mixed":
            assert ((hits["hit"] != 0) & (hits["prim_id"] >= sd.ntris) & (hits["prim_id"] < sd.ntris + 2)).sum() >= 1, "sphere hits"
        rng = np.random.default_rng(C)
        g = _values(rng, (n, C))
        g[~ok] = np.nan
        init = _values(rng, (_nverts(sd), C))
        w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
        ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
        table = Guarded(init.shape)
        table.t.copy_(_dev(init))
        sc.interpolate_hits_grad_tensor(_dev_rays(rays), _dev_hits(hits), _dev(g), grad_attr=table.t)
        got = _np(table.t)
        beyond, touched = gr.check(got, ref, S, m, f"{name} C={C} list")
        assert touched > 0 and beyond <= 0.02 * touched, (beyond, touched)
        assert _bits_equal(got[m == 0], init[m == 0]), "rows no valid item names keep their bytes"
        assert table.intact()
        host = sc.interpolate_hits_grad(rays, hits, g, grad_attr=init.copy())
        gr.check(host, ref, S, m, f"{name} C={C} host form")
        assert _bits_equal(host[m == 0], init[m == 0])
    finally:
        if own:
            sc.close()


# ---- 4. frames ----
def _moved(pkg, W, H, i):
    cam = pkg.scenes.default_camera(W, H).copy()
    cam[3] += np.float32(0.3 * i)
    cam[4] += np.float32(0.5 * i)
    return cam


def _plane_hits(pkg, depth, prim):
    h = _hits(pkg, depth.reshape(-1), prim.reshape(-1).view(np.uint32))
    h["hit"] = h["prim_id"] != pkg.NO_PRIM
    return h


def _check_frames(pkg, sd, grad, cams, rays, W, H, depth, prim, chw, what):
    """grad(cams, W, H, depth, prim_id, grad_out, chw=, grad_attr=) against the restatement on the regenerated rays `rays` (B * H * W,
    view after view) and the planes' hits."""
    B = len(rays) // (W * H)
    hits = _plane_hits(pkg, _np(depth), _np(prim))
    ok = sr.triangle_mask(sd, hits["hit"], hits["prim_id"])
    assert ok.any() and not ok.all(), what
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    for C in (3, 32):
        rng = np.random.default_rng(C)
        g = _values(rng, (len(rays), C))
        g[~ok] = np.nan
        init = _values(rng, (_nverts(sd), C))
        ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
        g_dev = g.reshape(B, H, W, C)
        table = Guarded(init.shape)
        table.t.copy_(_dev(init))
        grad(cams, W, H, depth, prim, _dev(np.moveaxis(g_dev, -1, 1) if chw else g_dev), chw=chw, grad_attr=table.t)
        got = _np(table.t)
        beyond, touched = gr.check(got, ref, S, m, f"{what} C={C}")
        assert touched > 0 and beyond <= 0.02 * touched, (what, beyond, touched)
        assert _bits_equal(got[m == 0], init[m == 0]) and table.intact(), what


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 17), (72, 40)])
def test_trackball_frames(pkg, mixed, W, H, B, chw):
    sd, sc = mixed
    cams = np.stack([_moved(pkg, W, H, i) for i in range(B)])
    _, _, planes = sc.render_views_aov_tensor(cams, W, H, aovs=("depth", "prim_id"))
    rays = np.concatenate([sc.generate_rays(c, W, H) for c in cams])
    _check_frames(pkg, sd, sc.surface_views_grad_tensor, cams, rays, W, H, planes["depth"], planes["prim_id"], chw, ("trackball", W, H, B, chw))


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 17), (72, 40)])
def test_raycam_frames(pkg, mixed, W, H, B, chw):
    sd, sc = mixed
    cams = [pkg.RayCamera.from_trackball(_moved(pkg, W, H, i), W, H) for i in range(B - 1)]
    cams.append(pkg.RayCamera.from_trackball(_moved(pkg, 2 * W, 2 * H, B - 1), 2 * W, 2 * H).tile(W // 2, H // 3))
    _, _, planes = sc.render_raycams_tensor(cams, W, H, aovs=("depth", "prim_id"))
    rays = np.concatenate([sc.generate_rays_raycam(c, W, H) for c in cams])
    _check_frames(pkg, sd, sc.surface_raycams_grad_tensor, cams, rays, W, H, planes["depth"], planes["prim_id"], chw, ("raycam", W, H, B, chw))


def test_anti_aliased_planes(pkg, mixed):
    sd, sc = mixed
    W, H = 33, 17
    cam = _moved(pkg, W, H, 1)
    _, _, planes = sc.render_aov_tensor(cam, W, H, aovs=("depth", "prim_id"), aa=True)
    assert tuple(planes["depth"].shape) == (2 * H, 2 * W)
    rays = sc.generate_rays(cam, 2 * W, 2 * H)  # finding AA3: the sub-sample rays are the 2W x 2H frame's
    grad = lambda cams, w, h, d, p, g, chw, grad_attr: sc.surface_views_grad_tensor(cams, w, h, d, p, g[0], chw=chw, grad_attr=grad_attr)  # noqa: E731
    _check_frames(pkg, sd, grad, cam, rays, 2 * W, 2 * H, planes["depth"], planes["prim_id"], False, "aa planes, one camera, (H, W)")


# ---- 5. autograd ----
def _composition(sd, bary, prim, ok, table):
    """What a caller composes in torch from the barycentrics: three gathers and a weighted sum (its autograd: three index_add_)."""
    tri = _dev(np.asarray(sd.tri, np.int64).reshape(-1, 3))
    rows = tri[prim.clamp(0, sd.ntris - 1)]
    v = (bary[:, 0:1] * table[rows[:, 0]] + bary[:, 1:2] * table[rows[:, 1]]) + bary[:, 2:3] * table[rows[:, 2]]
    return torch.where(ok[:, None], v, torch.zeros((), dtype=torch.float32, device="cuda"))


def _autograd_case(pkg, sd, sc, kind):
    """(forward(attr, **kw) -> the attribute output, its item-major view, rays, hits) for one of the three tensor entries."""
    W, H = 33, 17
    if kind == "list":
        rays, hits = _capped_list(pkg, sd, sc, 1500, 41)
        d_rays, d_hits = _dev_rays(rays), _dev_hits(hits)
        return (lambda attr, **kw: sc.interpolate_hits_tensor(d_rays, d_hits, attr, **kw)), rays, hits, (len(rays),)
    if kind == "views":
        cams = np.stack([_moved(pkg, W, H, i) for i in range(2)])
        _, _, planes = sc.render_views_aov_tensor(cams, W, H, aovs=("depth", "prim_id"))
        rays = np.concatenate([sc.generate_rays(c, W, H) for c in cams])
        surface = sc.surface_views_tensor
    else:
        cams = [pkg.RayCamera.from_trackball(_moved(pkg, W, H, i), W, H) for i in range(2)]
        _, _, planes = sc.render_raycams_tensor(cams, W, H, aovs=("depth", "prim_id"))
        rays = np.concatenate([sc.generate_rays_raycam(c, W, H) for c in cams])
        surface = sc.surface_raycams_tensor
    hits = _plane_hits(pkg, _np(planes["depth"]), _np(planes["prim_id"]))

    def forward(attr, **kw):
        out = kw.pop("out", None)
        res = surface(cams, W, H, planes["depth"], planes["prim_id"], attr=attr, want_bary=False, **({"out": {"attr": out}} if out is not None else {}), **kw)
        return res["attr"]

    forward.full = lambda attr: surface(cams, W, H, planes["depth"], planes["prim_id"], attr=attr, want_bary=True)
    return forward, rays, hits, (2, H, W)


@pytest.mark.parametrize("kind", ["list", "views", "raycams"])
def test_autograd(pkg, mixed, kind):
    sd, sc = mixed
    forward, rays, hits, lead = _autograd_case(pkg, sd, sc, kind)
    C = 4
    rng = np.random.default_rng(8)
    table = _values(rng, (_nverts(sd), C))
    g = _values(rng, (len(rays), C))
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g)
    assert m.max() <= gr.M_CAP and m.sum() > 0
    attr = _dev(table).requires_grad_()
    d_g = _dev(g.reshape(lead + (C,)))
    out = forward(attr)
    assert out.requires_grad and out.grad_fn is not None and tuple(out.shape) == lead + (C,)
    plain = forward(attr.detach())
    assert not plain.requires_grad and _bits_equal(_np(out.detach()), _np(plain)), "the forward bytes are the non-recording call's"
    with torch.no_grad():
        assert not forward(attr).requires_grad, "grad mode off: the ordinary path"
    out.backward(d_g)
    first = _np(attr.grad).copy()
    gr.check(first, ref, S, m, f"autograd {kind}")
    assert not first[m == 0].any()
    # the torch composition's autograd: another order of the same rounded products
    t2 = _dev(table).requires_grad_()
    ok = _dev(sr.triangle_mask(sd, hits["hit"], hits["prim_id"]))
    comp = _composition(sd, _dev(w), _dev(hits["prim_id"].astype(np.int64)), ok, t2)
    assert _bits_equal(_np(comp.detach()), _np(plain).reshape(-1, C)), "the composition is the forward, bit for bit"
    comp.backward(d_g.reshape(-1, C))
    gr.check(_np(t2.grad), ref, S, m, f"torch composition {kind}")
    assert (np.abs(first.astype(np.float64) - _np(t2.grad)) <= 2 * gr.bound(S, m)).all()
    # a second backward accumulates: torch adds the new gradient (within the bound of ref) to the first, one more rounding
    forward(attr).backward(d_g)
    second = _np(attr.grad).astype(np.float64)
    assert (np.abs(second - 2 * ref) <= 2 * gr.bound(S, m) + gr.U * np.abs(second)).all()
    # out= with a table that requires grad
    with pytest.raises(ValueError):
        forward(attr, out=torch.empty(lead + (C,), dtype=torch.float32, device="cuda"))
    if kind != "list":
        res = forward.full(attr)
        assert res["attr"].requires_grad and not res["bary"].requires_grad, "'bary' is marked non-differentiable"
        assert _bits_equal(_np(res["bary"]).reshape(-1, 3), w) and _bits_equal(_np(res["attr"].detach()), _np(plain))
    # deterministic mode: the order of the sum is unspecified
    try:
        torch.use_deterministic_algorithms(True)
        with pytest.raises(RuntimeError, match="order"):
            forward(attr).backward(d_g)
        torch.use_deterministic_algorithms(True, warn_only=True)
        with pytest.warns(UserWarning, match="order"):
            forward(attr).backward(d_g)
    finally:
        torch.use_deterministic_algorithms(False)


def test_one_sgd_step_lowers_the_loss(pkg, mixed):
    sd, sc = mixed
    W, H = 72, 40
    cam = _moved(pkg, W, H, 0)
    _, _, planes = sc.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
    surface = lambda t: sc.surface_views_tensor(cam, W, H, planes["depth"][0], planes["prim_id"][0], attr=t, want_bary=False)["attr"]  # noqa: E731
    rng = np.random.default_rng(3)
    target = surface(_dev(rng.random((_nverts(sd), 3)).astype(np.float32)))
    colours = torch.nn.Parameter(torch.full((_nverts(sd), 3), 0.5, dtype=torch.float32, device="cuda"))
    # loss = |A x - y|^2; the largest eigenvalue of A^T A is at most its largest absolute row sum, max_v sum_i w_iv (sum_v' w_iv'):
    # evaluated with the adjoint itself, A^T (A 1).  Half the step that bound allows.
    with torch.no_grad():
        ones = torch.ones_like(colours)
        lam = float(sc.surface_views_grad_tensor(cam, W, H, planes["depth"][0], planes["prim_id"][0], surface(ones)).max())
    assert lam > 0
    opt = torch.optim.SGD([colours], lr=0.5 / (2 * lam))
    loss = ((surface(colours) - target) ** 2).sum()
    loss.backward()
    opt.step()
    with torch.no_grad():
        after = ((surface(colours) - target) ** 2).sum()
    print("loss", float(loss.detach()), "->", float(after))
    assert float(after) < float(loss.detach())


# ---- 6. streams and threads ----
def test_streams_and_threads(pkg, mixed, square):
    sd, sc = mixed
    sq_sd, sq_sc = square
    C = 6
    rng = np.random.default_rng(12)
    all_rays, all_hits = _capped_list(pkg, sd, sc, 1200, 51)
    jobs = []
    for k in range(8):
        if k % 2:
            rays, hits = _square_list(pkg, _order("runs", 37 + 40 * k, rng))
            g = rng.integers(-8, 9, (len(rays), C)).astype(np.float32)
            jobs.append((sq_sd, sq_sc, rays, hits, g))
        else:
            sl = slice(100 * k, 100 * k + 237 + 11 * k)
            g = _values(rng, (sl.stop - sl.start, C))
            jobs.append((sd, sc, all_rays[sl], all_hits[sl], g))
    dev = [(_dev_rays(r), _dev_hits(h), _dev(g)) for _, _, r, h, g in jobs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got, errors = {}, []

    def work(tid):
        try:
            for it in range(4):
                for k in range(tid, len(jobs), 4):
                    s = streams[(tid + it + k) % 2]
                    got[(tid, it, k)] = jobs[k][1].interpolate_hits_grad_tensor(*dev[k], stream=s)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    assert len(got) == 4 * len(jobs)
    for (tid, it, k), t in got.items():
        jsd, _, rays, hits, g = jobs[k]
        if k % 2:
            assert _bits_equal(t.cpu().numpy(), _exact(jsd, rays, hits, g, None)[0]), (tid, it, k)
        else:
            w = sr.weights(jsd, rays, hits["t"], hits["prim_id"], hits["hit"])
            gr.check(t.cpu().numpy(), *gr.adjoint(jsd, w, hits["prim_id"], hits["hit"], g), f"thread {tid} pass {it} job {k}")


# ---- 7. nothing else moves ----
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
        nverts = _nverts(sd)
        g = _values(np.random.default_rng(4), (500, 7))
        _, _, planes = a.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
        base = a.device_bytes()
        # n == 0 succeeds and touches nothing: no table either
        a.interpolate_hits_grad_device(0, 0, 0, 0, 7, 0)
        empty = a.interpolate_hits_grad_tensor(torch.empty((0, 7), device="cuda"), torch.empty((0, 4), dtype=torch.int32, device="cuda"),
                                               torch.empty((0, 7), device="cuda"))
        assert tuple(empty.shape) == (nverts, 7) and not _np(empty).any() and a.device_bytes() == base
        # the first gradient call builds the table a forward call would
        a.interpolate_hits_grad(rays, hits, g)
        assert a.device_bytes() == base + 16 * sd.ntris, "the lookup table, 16 bytes per triangle"
        attr = np.random.default_rng(5).standard_normal((nverts, 7)).astype(np.float32)
        fwd = a.interpolate_hits(rays, hits, attr)
        d_attr = _dev(attr)
        fwd_frame = _np(a.surface_views_tensor(cam, W, H, planes["depth"][0], planes["prim_id"][0], attr=d_attr)["attr"])
        table = a.interpolate_hits_grad_tensor(_dev_rays(rays), _dev_hits(hits), _dev(g))
        a.surface_views_grad_tensor(cam, W, H, planes["depth"][0], planes["prim_id"][0], torch.ones((H, W, 7), device="cuda"), grad_attr=table)
        a.surface_raycams_grad_tensor(pkg.RayCamera.from_trackball(cam, W, H), W, H, planes["depth"], planes["prim_id"],
                                      torch.ones((1, 7, H, W), device="cuda"), chw=True, grad_attr=table)
        torch.cuda.synchronize()
        assert same_bits(a.interpolate_hits(rays, hits, attr), fwd).all(), "forward outputs before and after gradient calls"
        assert same_bits(_np(a.surface_views_tensor(cam, W, H, planes["depth"][0], planes["prim_id"][0], attr=d_attr)["attr"]), fwd_frame).all()
        assert a.device_bytes() == base + 16 * sd.ntris, "once"
        ref = b.render(cam, W, H)
        for _ in range(2):
            ref = b.render(cam, W, H)
        b.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes() + 16 * sd.ntris, "a scene that makes no surface call keeps both"
    finally:
        a.close()
        b.close()

"""GPU tests of the bitwise-reproducible form of the table adjoint (include/cgrt.h cgrt_interpolate_hits_grad_repro*,
cgrt_surface_*_grad_repro_device; the reproducible=True keyword of Scene.interpolate_hits_grad and its *_device / *_tensor forms, of
surface_views_grad_tensor, surface_raycams_grad_tensor and of the three forward tensor entries).

The result is defined to the last bit, so the check is bytes against tests/surface_grad_repro_ref.py, the numpy restatement of the
header's definition, on the scenes and fixtures of tests/test_surface_grad_gpu.py; where that module's float64 bound applies the result
is held to it as well (the reproducible form is a legal value of the float form)."""
import threading
import warnings

import numpy as np
import pytest

import surface_grad_ref as gr
import surface_grad_repro_ref as rr
import surface_ref as sr
import test_surface_grad_gpu as tg
from test_surface_grad_gpu import KEYS, PAD, SENTINEL, Guarded, _bits_equal, _dev, _dev_hits, _dev_rays, _hits, _np, _nverts, _values
from test_surface_grad_gpu import mixed, soup, square  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _first_difference(got, want):
    d = np.argwhere(np.ascontiguousarray(got, np.float32).view(np.uint32) != np.ascontiguousarray(want, np.float32).view(np.uint32))
    return None if not len(d) else (len(d), d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])])


def _repro(sc, d_rays, d_hits, g, init):
    """The reproducible list entry on a guarded copy of init; returns the table's bytes."""
    table = Guarded(init.shape)
    table.t.copy_(_dev(init))
    got = sc.interpolate_hits_grad_tensor(d_rays, d_hits, g if isinstance(g, torch.Tensor) else _dev(g), grad_attr=table.t, reproducible=True)
    assert got is table.t
    res = _np(got).copy()
    assert table.intact()
    return res


# ---- 1. bytes ----
@pytest.fixture(scope="module")
def lists(pkg, scene_data, mixed):  # noqa: F811
    """Per scene: about 5 000 seeded rays with their hits (misses, spheres and out-of-range ids among them, no vertex beyond the
    float64 check's cap), the restated weights, and the device copies -- computed once for every channel count."""
    made, own = {}, []

    def get(name):
        if name not in made:
            if name == "mixed":
                sd, sc = mixed
            else:
                sd = scene_data(name)
                sc = pkg.Scene(sd, device=0)
                own.append(sc)
            rays, hits = tg._capped_list(pkg, sd, sc, 5003, 31)
            w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
            made[name] = (sd, sc, rays, hits, w, _dev_rays(rays), _dev_hits(hits))
        return made[name]

    yield get
    for sc in own:
        sc.close()


@pytest.mark.parametrize("C", [1, 3, 4, 5, 32, 33, 256])
@pytest.mark.parametrize("name", ["mixed", "monkey", "cornell"])
def test_bytes(pkg, lists, name, C):
    sd, sc, rays, hits, w, d_rays, d_hits = lists(name)
    ok = sr.triangle_mask(sd, hits["hit"], hits["prim_id"])
    assert ok.sum() >= 300 and (~ok).sum() >= 20, (name, int(ok.sum()))
    rng = np.random.default_rng(100 + C)
    g = _values(rng, (len(rays), C))
    g[~ok] = np.nan
    init = _values(rng, (_nverts(sd), C))
    want = rr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
    got = _repro(sc, d_rays, d_hits, g, init)
    assert _bits_equal(got, want), (name, C, _first_difference(got, want))
    ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
    beyond, touched = gr.check(got, ref, S, m, f"{name} C={C} reproducible list")
    assert touched > 0 and beyond == 0
    assert _bits_equal(got[m == 0], init[m == 0])
    if C in (3, 32):
        host = sc.interpolate_hits_grad(rays, hits, g, grad_attr=init.copy(), reproducible=True)
        assert _bits_equal(host, want), (name, C, "host form", _first_difference(host, want))


# ---- 2. order-free ----
@pytest.mark.parametrize("C", [3, 32])
def test_a_shuffled_list_and_a_second_call_give_the_same_bytes(pkg, lists, C):
    sd, sc, rays, hits, w, d_rays, d_hits = lists("mixed")
    rng = np.random.default_rng(7 + C)
    g = _values(rng, (len(rays), C))
    g[~sr.triangle_mask(sd, hits["hit"], hits["prim_id"])] = np.nan
    init = _values(rng, (_nverts(sd), C))
    first = _repro(sc, d_rays, d_hits, g, init)
    assert _bits_equal(_repro(sc, d_rays, d_hits, g, init), first), "the call made twice"
    for _ in range(2):
        p = rng.permutation(len(rays))
        again = _repro(sc, _dev_rays(rays[p]), _dev_hits(hits[p]), g[p], init)
        assert _bits_equal(again, first), (C, "shuffled", _first_difference(again, first))


@pytest.mark.parametrize("C", [1, 5, 32])
@pytest.mark.parametrize("kind", ["one_triangle", "runs"])
def test_contended_rows_give_the_exact_value(pkg, square, kind, C):  # noqa: F811
    sd, sc = square
    rng = np.random.default_rng(400 + C)
    n = 4099
    idx = tg._order(kind, n, rng)
    rays, hits = tg._square_list(pkg, idx)
    g = rng.integers(-8, 9, (n, C)).astype(np.float32)
    init = rng.integers(-8, 9, (4, C)).astype(np.float32)
    want, m = tg._exact(sd, rays, hits, g, init)
    assert kind != "one_triangle" or sorted(m.tolist()) == [0, n, n, n], "three destination rows"
    first = _repro(sc, _dev_rays(rays), _dev_hits(hits), g, init)
    assert _bits_equal(first, want), (kind, C, _first_difference(first, want))
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    assert _bits_equal(rr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init), want), "the restatement is exact here too"
    assert _bits_equal(_repro(sc, _dev_rays(rays), _dev_hits(hits), g, init), first), "twice"
    p = rng.permutation(n)
    assert _bits_equal(_repro(sc, _dev_rays(rays[p]), _dev_hits(hits[p]), g[p], init), first), "shuffled"


# ---- 3. reduced S and truncation ----
@pytest.mark.parametrize("C", [3, 32])
def test_reduced_shift_and_truncated_terms(pkg, square, C):  # noqa: F811
    sd, sc = square
    n, nvalid = 1 << 20, 4096
    assert rr.shift(n) == 16
    rng = np.random.default_rng(90 + C)
    at = np.sort(rng.choice(n, nvalid, replace=False))
    vr, vh = tg._square_list(pkg, np.repeat(rng.integers(0, len(tg.PTS), nvalid // 2), 2))  # pairs of items at one point
    rays = np.zeros((n, 7), np.float32)
    rays[:, 5], rays[:, 6] = -1.0, tg.FLT_MAX
    rays[at] = vr
    hits = _hits(pkg, 1.0, np.zeros(n, np.uint32), hit=0)
    hits[at] = vh
    ex = rng.integers(-40, 41, (nvalid, C))
    ex[1::2] = np.minimum(ex[1::2], 10)
    gv = (np.where(rng.random((nvalid, C)) < 0.5, -1.0, 1.0) * rng.uniform(1, 2, (nvalid, C)) * 2.0 ** ex).astype(np.float32)
    # the large values cancel pair by pair, exactly: they set E, and what is left of the sum are the terms the shift cuts into
    gv[1::2] = np.where(ex[0::2] > 10, -gv[0::2], gv[1::2])
    g = np.full((n, C), np.nan, np.float32)
    g[at] = gv
    init = _values(rng, (4, C))
    w = sr.weights(sd, vr, vh["t"], vh["prim_id"], vh["hit"])
    # the case is what it claims to be: terms shifted right, and terms shifted out altogether
    dest, x = rr.contributions(sd, w, vh["prim_id"], vh["hit"], gv, C)
    e = np.maximum((x.view(np.uint32) >> 23) & 0xFF, 1).astype(np.int64)
    E = np.zeros(4 * C, np.int64)
    np.maximum.at(E, dest, e)
    d = E[dest] - e
    assert ((d > 16) & (d < 40)).any() and (d >= 40).any()
    want = rr.adjoint(sd, w, vh["prim_id"], vh["hit"], gv, init, n=n)
    assert not _bits_equal(want, rr.adjoint(sd, w, vh["prim_id"], vh["hit"], gv, init)), "S matters on these inputs"
    got = _repro(sc, _dev_rays(rays), _dev_hits(hits), g, init)
    assert _bits_equal(got, want), (C, _first_difference(got, want))


# ---- 4. frames ----
def _frame_case(pkg, sd, sc, raycams, cams, rays, W, H, depth, prim, chw):
    B = len(rays) // (W * H)
    hits = tg._plane_hits(pkg, _np(depth), _np(prim))
    ok = sr.triangle_mask(sd, hits["hit"], hits["prim_id"])
    assert ok.any() and not ok.all()
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    grad = sc.surface_raycams_grad_tensor if raycams else sc.surface_views_grad_tensor
    d_rays, d_hits = _dev_rays(rays), _dev_hits(hits)
    for C in (3, 32):
        rng = np.random.default_rng(C)
        g = _values(rng, (len(rays), C))
        g[~ok] = np.nan
        init = _values(rng, (_nverts(sd), C))
        want = rr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
        g_dev = g.reshape(B, H, W, C)
        table = Guarded(init.shape)
        table.t.copy_(_dev(init))
        grad(cams, W, H, depth, prim, _dev(np.moveaxis(g_dev, -1, 1) if chw else g_dev), chw=chw, grad_attr=table.t, reproducible=True)
        got = _np(table.t)
        assert _bits_equal(got, want) and table.intact(), (raycams, W, H, B, chw, C, _first_difference(got, want))
        as_list = _repro(sc, d_rays, d_hits, g, init)  # the same n, hence the same S
        assert _bits_equal(as_list, got), (raycams, W, H, B, chw, C, "the list entry on the frame's rays and hits")


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 17), (72, 40)])
def test_trackball_frames(pkg, mixed, W, H, B, chw):  # noqa: F811
    sd, sc = mixed
    cams = np.stack([tg._moved(pkg, W, H, i) for i in range(B)])
    _, _, planes = sc.render_views_aov_tensor(cams, W, H, aovs=("depth", "prim_id"))
    rays = np.concatenate([sc.generate_rays(c, W, H) for c in cams])
    _frame_case(pkg, sd, sc, False, cams, rays, W, H, planes["depth"], planes["prim_id"], chw)


@pytest.mark.parametrize("chw", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,H", [(33, 17), (72, 40)])
def test_raycam_frames(pkg, mixed, W, H, B, chw):  # noqa: F811
    sd, sc = mixed
    cams = [pkg.RayCamera.from_trackball(tg._moved(pkg, W, H, i), W, H) for i in range(B - 1)]
    cams.append(pkg.RayCamera.from_trackball(tg._moved(pkg, 2 * W, 2 * H, B - 1), 2 * W, 2 * H).tile(W // 2, H // 3))
    _, _, planes = sc.render_raycams_tensor(cams, W, H, aovs=("depth", "prim_id"))
    rays = np.concatenate([sc.generate_rays_raycam(c, W, H) for c in cams])
    _frame_case(pkg, sd, sc, True, cams, rays, W, H, planes["depth"], planes["prim_id"], chw)


# ---- 5. non-finite and subnormal ----
@pytest.mark.parametrize("C", [4, 33])
def test_non_finite_rows_follow_the_rule(pkg, soup, C):  # noqa: F811
    """Triangles that share no vertex, three items each: item 0 of triangle k carries the special row, so the three rows of triangle
    k's vertices show the rule and every other row shows that nothing leaks."""
    sd, sc, rays1, hits1 = soup
    T = len(rays1)
    rays, hits = np.concatenate([rays1] * 3), np.concatenate([hits1] * 3)
    rng = np.random.default_rng(C)
    g = _values(rng, (3 * T, C))
    inf = np.float32(np.inf)
    g[0] = inf                      # triangle 0: +inf
    g[1] = -inf                     # triangle 1: -inf
    g[2], g[T + 2] = inf, -inf      # triangle 2: both
    g[3] = np.nan                   # triangle 3: NaN
    g[4], g[T + 4] = np.nan, inf    # triangle 4: NaN and an infinity
    g[5, 0] = inf                   # triangle 5: one channel only
    for k in (6, 7, 8, 9):          # the same rows behind invalid items stay out
        hits["hit"][k] = 0
    g[6], g[7], g[8] = inf, -inf, np.nan
    hits["prim_id"][T + 9] = sd.ntris + 5
    g[T + 9] = np.nan
    init = _values(rng, (_nverts(sd), C))
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    init[tri[0, 1]] = -inf          # previous content -inf meets +inf: NaN
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    want = rr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
    got = _repro(sc, _dev_rays(rays), _dev_hits(hits), g, init)
    assert _bits_equal(got, want), (C, _first_difference(got, want))
    bits = got.view(np.uint32)
    assert (got[tri[0, [0, 2]]] == inf).all() and (bits[tri[0, 1]] == rr.QNAN).all()
    assert (got[tri[1]] == -inf).all()
    assert (bits[tri[2]] == rr.QNAN).all() and (bits[tri[3]] == rr.QNAN).all() and (bits[tri[4]] == rr.QNAN).all()
    assert (got[tri[5], 0] == inf).all() and np.isfinite(got[tri[5], 1:]).all()
    assert np.isfinite(got[tri[6:]]).all(), "rows of invalid items and of every other triangle stay finite"


@pytest.mark.parametrize("e", [-130, -140])
@pytest.mark.parametrize("C", [3, 32])
def test_subnormal_sums_are_exact(pkg, square, C, e):  # noqa: F811
    sd, sc = square
    rng = np.random.default_rng(C - e)
    n = 320
    rays, hits = tg._square_list(pkg, rng.integers(0, len(tg.PTS), n))
    scale = np.float32(2.0**e)
    g = rng.integers(-8, 9, (n, C)).astype(np.float32) * scale
    init = rng.integers(-8, 9, (4, C)).astype(np.float32) * scale
    want, _ = tg._exact(sd, rays, hits, g, init)
    assert (np.abs(g) < 2.0**-126).all() and (np.abs(want[want != 0]) < 2.0**-126).any(), "subnormal contributions, subnormal images"
    got = _repro(sc, _dev_rays(rays), _dev_hits(hits), g, init)
    assert _bits_equal(got, want), (C, e, _first_difference(got, want))


# ---- 6. what must not move ----
def test_nothing_else_moves(pkg, scene_data):
    sd = scene_data("cornell")
    a, b = pkg.Scene(sd, device=0), pkg.Scene(sd, device=0)
    try:
        W, H, C = 64, 48, 7
        cam = pkg.scenes.default_camera(W, H)
        for _ in range(3):
            before = a.render(cam, W, H)
        path = a.last_render_path()
        rays = sr.random_rays(sd, 500, 9)
        hits, _ = a.intersect(rays)
        nverts = _nverts(sd)
        rng = np.random.default_rng(4)
        g = _values(rng, (500, C))
        _, _, planes = a.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
        base = a.device_bytes()
        # n == 0 succeeds and touches nothing: no lookup table, no workspace needed
        a.interpolate_hits_grad_device(0, 0, 0, 0, C, 0, reproducible=True)
        empty = a.interpolate_hits_grad_tensor(torch.empty((0, 7), device="cuda"), torch.empty((0, 4), dtype=torch.int32, device="cuda"),
                                               torch.empty((0, C), device="cuda"), reproducible=True)
        assert tuple(empty.shape) == (nverts, C) and not _np(empty).any() and a.device_bytes() == base
        # rows no valid item names keep their bytes: distinct NaN payloads; guards around the table and around the workspace
        w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
        ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g)
        assert (m == 0).any() and (m > 0).any() and m.max() <= gr.M_CAP
        init = np.zeros((nverts, C), np.float32)
        init[m > 0] = _values(rng, (int((m > 0).sum()), C))
        payload = (np.uint32(0x7FC00001) + np.arange(int((m == 0).sum()) * C, dtype=np.uint32)).reshape(-1, C)
        init.view(np.uint32)[m == 0] = payload
        table = Guarded(init.shape)
        table.t.copy_(_dev(init))
        nbytes = a.surface_grad_repro_workspace(C)
        assert nbytes == 12 * nverts * C
        ws = torch.full((nbytes + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
        d_rays, d_hits, d_g = _dev_rays(rays), _dev_hits(hits), _dev(g)
        torch.cuda.synchronize()
        a.interpolate_hits_grad_device(d_rays.data_ptr(), d_hits.data_ptr(), 500, d_g.data_ptr(), C, table.t.data_ptr(),
                                       stream=torch.cuda.current_stream().cuda_stream, reproducible=True, d_workspace_ptr=ws.data_ptr() + PAD,
                                       workspace_bytes=nbytes)
        got = _np(table.t)
        assert table.intact()
        edge = ws.cpu().numpy()
        assert (edge[:PAD] == SENTINEL).all() and (edge[PAD + nbytes:] == SENTINEL).all(), "guard bytes around the workspace"
        assert (got.view(np.uint32)[m == 0] == payload).all(), "rows no valid item names, compared as bytes"
        want = rr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
        assert _bits_equal(got, want), _first_difference(got, want)
        assert a.device_bytes() == base + 16 * sd.ntris, "the lookup table a forward call would build, and nothing else"
        # the float entry on the same inputs lies within its bound of the reproducible one
        zero = np.zeros((nverts, C), np.float32)
        repro = _repro(a, d_rays, d_hits, g, zero)
        flt = _np(a.interpolate_hits_grad_tensor(d_rays, d_hits, d_g))
        gr.check(repro, ref, S, m, "reproducible")
        gr.check(flt, ref, S, m, "float atomics")
        assert (np.abs(flt.astype(np.float64) - repro) <= 2 * gr.bound(S, m)).all()
        # frames through both cameras, then: the scene's stats, prediction record and a following frame
        tab = a.surface_views_grad_tensor(cam, W, H, planes["depth"][0], planes["prim_id"][0], torch.ones((H, W, C), device="cuda"), reproducible=True)
        a.surface_raycams_grad_tensor(pkg.RayCamera.from_trackball(cam, W, H), W, H, planes["depth"], planes["prim_id"],
                                      torch.ones((1, C, H, W), device="cuda"), chw=True, grad_attr=tab, reproducible=True)
        host = a.interpolate_hits_grad(rays, hits, g, reproducible=True)
        assert _bits_equal(host, repro), "host form, a new table"
        torch.cuda.synchronize()
        assert a.device_bytes() == base + 16 * sd.ntris, "once"
        ref_b = b.render(cam, W, H)
        for _ in range(2):
            ref_b = b.render(cam, W, H)
        b.render_views_aov_tensor(cam[None], W, H, aovs=("depth", "prim_id"))
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref_b[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes() + 16 * sd.ntris
    finally:
        a.close()
        b.close()


# ---- 7. autograd ----
@pytest.mark.parametrize("kind", ["list", "views", "raycams"])
def test_autograd_in_deterministic_mode(pkg, mixed, kind):  # noqa: F811
    sd, sc = mixed
    forward, rays, hits, lead = tg._autograd_case(pkg, sd, sc, kind)
    C = 4
    rng = np.random.default_rng(8)
    table = _values(rng, (_nverts(sd), C))
    g = _values(rng, (len(rays), C))
    d_g = _dev(g.reshape(lead + (C,)))
    w = sr.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])
    want = rr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, np.zeros_like(table))
    direct = _repro(sc, _dev_rays(rays), _dev_hits(hits), g, np.zeros_like(table))
    assert _bits_equal(direct, want), _first_difference(direct, want)
    plain = _np(forward(_dev(table)))
    grads = []
    try:
        torch.use_deterministic_algorithms(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for _ in range(2):
                attr = _dev(table).requires_grad_()
                out = forward(attr, reproducible=True)
                assert out.requires_grad and _bits_equal(_np(out.detach()), plain), "the forward is the same either way"
                out.backward(d_g)
                grads.append(_np(attr.grad).copy())
        # without the keyword nothing changes: the float backward still refuses
        with pytest.raises(RuntimeError, match="order"):
            forward(_dev(table).requires_grad_()).backward(d_g)
    finally:
        torch.use_deterministic_algorithms(False)
    assert _bits_equal(grads[0], direct), (kind, _first_difference(grads[0], direct))
    assert _bits_equal(grads[1], grads[0]), "two backward passes"


# ---- 8. streams and threads ----
def test_streams_and_threads(pkg, lists):
    sd, sc, rays, hits, w, d_rays, d_hits = lists("mixed")
    rng = np.random.default_rng(12)
    jobs = []
    for k in range(8):
        C = (3, 32, 5, 64)[k % 4]
        sl = slice(300 * k, 300 * k + 1500 + 37 * k)
        g = _values(rng, (sl.stop - sl.start, C))
        g[~sr.triangle_mask(sd, hits["hit"][sl], hits["prim_id"][sl])] = np.nan
        jobs.append((d_rays[sl], d_hits[sl], _dev(g)))
    serial = [_np(sc.interpolate_hits_grad_tensor(*j, reproducible=True)).copy() for j in jobs]
    sl = slice(0, 1500)
    assert _bits_equal(serial[0], rr.adjoint(sd, w[sl], hits["prim_id"][sl], hits["hit"][sl], _np(jobs[0][2]), np.zeros_like(serial[0])))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got, errors = {}, []

    def work(tid):
        try:
            for it in range(4):
                for k in range(tid, len(jobs), 4):
                    s = streams[(tid + it + k) % 2]
                    got[(tid, it, k)] = sc.interpolate_hits_grad_tensor(*jobs[k], stream=s, reproducible=True)  # (a workspace each)
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
        assert _bits_equal(t.cpu().numpy(), serial[k]), (tid, it, k)

"""GPU tests of the surface family across scale: the barycentric weights and the rows mixed with them (k_surface: include/cgrt.h
cgrt_hit_barycentrics*, cgrt_interpolate_hits*, cgrt_surface_raycams_device), their gradients (k_surface_grad; 5.23) and
the surface samples (k_sample_surface; 5.27).  Scene, ray origins, t and depth are multiplied by 2^k, k in test_surface_scale_cpu.KS.  None
of the three kernels walks the tree, so every input is made on the CPU without a tracer (scale_ref.surface_items).

* Weights at EVERY k, inside and outside the envelope: the device form equals surface_ref.weights of the scaled items bit for bit, on five
  scenes, among subnormal differences, products and areas (2^-70, 2^-75) and among inf and NaN (2^64, 2^66); the host form on cube and
  dodge at 2^-70 and 2^64.  A flushed subnormal, a conversion between f32 and f64 that treats a subnormal as zero, a division or a
  narrowing that is not correctly rounded for subnormal operands or results fails here.
* Covariance: wherever scale_ref.in_surface_envelope says inside, the device's weights at 2^k are the device's weights at 1, by bits; at
  2^-31 and 2^63 that is every item.
* Rows: interpolate_hits_tensor equals surface_ref.mix of the restated weights by bits at every k, for C = 3, 4, 7 (the scalar and the
  16-byte path), with a seeded table, with the scaled vertex positions themselves (padded with zeros), whose products overflow at 2^64,
  and with the seeded table times 2^-136, whose entries, products and sums are subnormal (the positions alone do not get there: a
  coordinate of 2^-70 times a weight near 1 is still normal).
* Frames without a tracer: the unit-square ray-camera frame of test_surface_grad_gpu.py, camera origin fields, depth and scene times 2^k.
* Samples at every k: sample_surface_device equals sampling_ref.sample of the scaled scene by bytes, independent and stratified, also
  where the scene has become empty for sampling (miss records, zero rows), where areas vanish or overflow, where `last` has moved and
  where one threshold repeats thousands of times; with the scaled positions as the table the rows are the points.
* Gradients: what global_atomic_add_f32 does with subnormals, observed on sums that are exact in every order and asserted as include/cgrt.h
  ("Order") then states it; and real items at 2^-31, 1 and 2^62 against the bound of tests/surface_grad_ref.py."""
import numpy as np
import pytest

import raycam_ref
import sampling_ref as sref
import scale_ref as sr
import surface_grad_ref as gr
import surface_ref
from conftest import same_bits
from test_surface_gpu import _dev_hits, _dev_rays, _np, _out, _same
from test_surface_grad_gpu import MAPS, PTS, Guarded, _dev, _hits, _order, _square_list, _values
from test_surface_scale_cpu import ALL_INSIDE, EXTRA_KS, FRAME_KS, KS, N, SAME_TABLE, SCENES, SEED, TABLE_SCENES, unit_square

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHANNELS = (3, 4, 7)
HOST_FORM = (("cube", -70), ("cube", 64), ("dodge", -70), ("dodge", 64))
FRAME_EXACT_KS = (-31, 30, 62)  # the weights are the thirty-seconds of scale 1
SAMPLE_SEED = 3
GRAD_KS = (-31, 0, 62)
EXPONENTS = (0, -120, -130, -140)

_data = {}
_scenes = {}


@pytest.fixture(scope="module")
def world(pkg, scene_data):
    """get(name, k) -> (scaled SceneData, Scene on device 0, scaled rays, prim, hit records), each made once; get.measures(name): the
    items' scale_ref.surface_measures at scale 1."""

    def data(name):
        if name not in _data:
            sd = unit_square(pkg) if name == "square" else scene_data(name)
            rays, prim = sr.surface_items(sd, N, SEED)
            _data[name] = (sd, rays, prim, sr.surface_measures(sd, rays, prim))
        return _data[name]

    def get(name, k):
        sd, rays, prim, _ = data(name)
        if (name, k) not in _scenes:
            sk = sr.scaled(sd, k)
            _scenes[(name, k)] = (sk, pkg.Scene(sk, device=0))
        sk, sc = _scenes[(name, k)]
        rk = sr.scaled_rays(rays, k)
        return sk, sc, rk, prim, _hits(pkg, rk[:, 6], prim)

    get.measures = lambda name: data(name)[3]
    yield get
    for _, sc in _scenes.values():
        sc.close()
    _scenes.clear()


def _restated(sd, rays, hits):
    return surface_ref.weights(sd, rays, hits["t"], hits["prim_id"], hits["hit"])


def _device_weights(sc, rays, hits):
    g, out = _out((len(rays), 3))
    got = sc.hit_barycentrics_tensor(_dev_rays(rays), _dev_hits(hits), out=out)
    assert got is out
    w = _np(out)
    assert g.intact()
    return w


def _first_difference(got, want):
    bad = np.flatnonzero(~same_bits(got, want).reshape(len(got), -1).all(axis=1))
    return (len(bad),) + ((int(bad[0]), got[bad[0]], want[bad[0]]) if len(bad) else ())


# ---- 1. weights at every k ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCENES)
def test_weights_equal_the_restatement_at_every_k(pkg, world, name, k):
    sd, sc, rays, prim, hits = world(name, k)
    ref = _restated(sd, rays, hits)
    got = _device_weights(sc, rays, hits)
    assert _same(got, ref), (name, k, "device form") + _first_difference(got, ref)
    if (name, k) in HOST_FORM:
        host = sc.hit_barycentrics(rays, hits)
        assert _same(host, ref), (name, k, "host form") + _first_difference(host, ref)
    if k == -70:
        sd0, _, rays0, _, hits0 = world(name, 0)
        assert not sr.in_surface_envelope(world.measures(name), k).any(), "every item has a subnormal cross product at 2^-70"
        assert (~sr.covariant_weights(_restated(sd0, rays0, hits0), ref)).mean() > 0.9, "and its weights are not those of scale 1"
    if k == 64 and name == "cube":
        assert np.isnan(ref).any(), "the sweep reaches NaN weights"


# ---- 2. covariance on the device ----
@pytest.mark.parametrize("name", SCENES)
def test_device_weights_are_covariant_inside_the_envelope(pkg, world, name):
    _, sc0, rays0, _, hits0 = world(name, 0)
    w0 = _device_weights(sc0, rays0, hits0)
    measures = world.measures(name)
    for k in KS:
        if k == 0:
            continue
        env = sr.in_surface_envelope(measures, k)
        if k in ALL_INSIDE:  # (-31 and 63 among them: the non-vacuity line of the CPU module)
            assert env.all(), (name, k, "items outside the envelope", int((~env).sum()))
        if not env.any():
            continue
        _, sc, rays, _, hits = world(name, k)
        wk = _device_weights(sc, rays, hits)
        bad = np.flatnonzero(env & ~sr.covariant_weights(w0, wk))
        print(f"{name}, 2^{k}: {int(env.sum())} of {N} items inside the envelope")
        assert len(bad) == 0, (name, k, "not the bits of scale 1 inside the envelope", len(bad), int(bad[0]), w0[bad[0]], wk[bad[0]])


# ---- 3. rows ----
def _tables(sd, C):
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    seeded = _values(np.random.default_rng(100 + C), (nverts, C))
    pos = np.zeros((nverts, C), np.float32)
    pos[:, 0:3] = np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3]
    with np.errstate(all="ignore"):
        tiny = np.ldexp(seeded, -136)  # |x| in [2^-146, 2^-126]: subnormal entries, products and sums, whatever k is
    return (("seeded", seeded), ("positions", pos), ("subnormal", tiny))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCENES)
def test_rows_equal_the_mix_of_the_restated_weights(pkg, world, name, k):
    sd, sc, rays, prim, hits = world(name, k)
    w = _restated(sd, rays, hits)
    d_rays, d_hits = _dev_rays(rays), _dev_hits(hits)
    for C in CHANNELS:
        for label, attr in _tables(sd, C):
            ref = surface_ref.mix(sd, w, hits["prim_id"], hits["hit"], attr)
            g, out = _out((len(rays), C))
            sc.interpolate_hits_tensor(d_rays, d_hits, torch.from_numpy(attr).cuda(), out=out)
            got = _np(out)
            assert _same(got, ref), (name, k, C, label) + _first_difference(got, ref)
            assert g.intact()
            if label == "subnormal" and k == 0:
                assert ((np.abs(ref) > 0) & (np.abs(ref) < sr.FLT_MIN)).mean() > 0.5, "the mix runs in the subnormal range"
            if label == "positions" and k in (64, 66) and name in ("cube", "cornell"):
                assert not np.isfinite(ref).all(), "the mix overflows"


# ---- 4. frames without a tracer ----
def _square_frame(pkg, world, k):
    """The 16 x 16 unit-square frame of test_surface_grad_gpu.py::test_exact_under_contention_frames with the camera's origin fields,
    the depth and the scene multiplied by 2^k: (scene data, scene, camera, depth plane, prim_id plane)."""
    sd, sc = world("square", k)[0:2]
    s = np.ldexp(1.0, k)
    cam = pkg.RayCamera.from_fields((s / 32, s / 32, s), (s / 16, 0, 0), (0, s / 16, 0), (0, 0, -1), (0, 0, 0), (0, 0, 0))
    y, x = np.mgrid[0:16, 0:16]
    prim = np.where(x + y < 15, 0, np.where(x + y == 15, pkg.NO_PRIM, 1)).astype(np.uint32)
    return sd, sc, cam, np.full((16, 16), s, np.float32), prim


@pytest.mark.parametrize("k", (0,) + FRAME_KS)
def test_unit_square_frames(pkg, world, k):
    W = H = 16
    sd, sc, cam, depth, prim = _square_frame(pkg, world, k)
    rays = sc.generate_rays_raycam(cam, W, H)
    assert _same(rays.view(np.float32).reshape(-1, 7), raycam_ref.rays_of(cam, W, H)), (k, "the rays of the scaled camera")
    hits = _hits(pkg, depth.reshape(-1), prim.reshape(-1))
    hits["hit"] = hits["prim_id"] != pkg.NO_PRIM
    ref = _restated(sd, rays, hits)
    g, out = _out((1, H, W, 3))
    res = sc.surface_raycams_tensor([cam], W, H, _dev(depth[None]), _dev(prim.view(np.int32)[None]), out={"bary": out})
    got = _np(res["bary"]).reshape(-1, 3)
    assert g.intact()
    assert _same(got, ref), (k, "frame form against the restatement") + _first_difference(got, ref)
    assert _same(got, _device_weights(sc, rays, hits)), (k, "frame form against the list form")
    ok = hits["hit"] != 0
    assert ok.sum() == 240 and not got[~ok].any()
    if k == 0 or k in FRAME_EXACT_KS:
        sd0, sc0, cam0, depth0, _ = _square_frame(pkg, world, 0)
        hits0 = hits.copy()
        hits0["t"] = depth0.reshape(-1)
        w0 = _restated(sd0, sc0.generate_rays_raycam(cam0, W, H), hits0)
        assert (w0 * 32 == np.round(w0 * 32)).all() and w0[ok].min() >= 1 / 32
        assert _same(got, w0), (k, "the thirty-seconds of scale 1")
    if k == 64:
        assert (ref[ok] == 0).all(), "the square's area overflows and the three others do not: finite / inf"


# ---- 5. samples at every k ----
def _device_samples(sc, n, attr=None, **kw):
    """(records, rows or None) of sample_surface_device, each output between guards."""
    g_rec, rec = _out((n, 8))
    if attr is None:
        sc.sample_surface_device(n, rec.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **kw)
        rows = None
    else:
        d_attr = torch.from_numpy(np.ascontiguousarray(attr, np.float32)).cuda()
        g_rows, rows = _out((n, attr.shape[1]))
        sc.sample_surface_device(n, rec.data_ptr(), d_attr_ptr=d_attr.data_ptr(), channels=attr.shape[1], d_out_attr_ptr=rows.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream, **kw)
        rows = _np(rows)
        assert g_rows.intact()
    rec = _np(rec).reshape(-1).view(sref.SAMPLE_DTYPE)
    assert g_rec.intact()
    return rec, rows


def _same_records(got, want, what):
    bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(axis=1))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("name,k", [(name, k) for name in TABLE_SCENES for k in KS + EXTRA_KS.get(name, ())])
def test_samples_equal_the_restatement_at_every_k(pkg, world, name, k):
    sd, sc = world(name, k)[0:2]
    tab = sref.table(sd)
    pos = np.ascontiguousarray(np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3])
    for strata in (0, N):
        want, want_rows = sref.sample(sd, N, seed=SAMPLE_SEED, strata=strata, attr=pos, tab=tab)
        rec, none = _device_samples(sc, N, seed=SAMPLE_SEED, strata=strata)
        assert none is None
        _same_records(rec, want, (name, k, strata, "records"))
        rec, rows = _device_samples(sc, N, attr=pos, seed=SAMPLE_SEED, strata=strata)
        _same_records(rec, want, (name, k, strata, "records, with a table"))
        assert rows.tobytes() == want_rows.tobytes(), (name, k, strata, "rows")
        assert np.array_equal(rows.view(np.uint32), rec["point"].view(np.uint32)), (name, k, strata, "the positions as the table give the points")
        if tab[3] == sref.NO_PRIM:
            assert (rec["prim_id"] == pkg.NO_PRIM).all() and (rec["mesh_id"] == 0xFFFFFFFF).all() and not rec["point"].any() and not rec["bary"].any()
            assert not rows.view(np.uint32).any(), "zero rows in a scene that is empty for sampling"
        else:
            assert not (tab[0][rec["prim_id"]] == 0).any(), "a triangle whose area counts as 0 is never chosen"
        if name in SAME_TABLE.get(k, ()):
            rec0, _ = _device_samples(world(name, 0)[1], N, seed=SAMPLE_SEED, strata=strata)
            bad = np.flatnonzero(~sr.covariant_samples(rec0, rec, k))
            assert len(bad) == 0, (name, k, strata, "not the power-of-two image of the samples at scale 1", len(bad), int(bad[0]))
    # what the CPU module found at this (scene, k) is what the device was run on
    empty = tab[3] == sref.NO_PRIM
    assert empty == (k == -75 or (name == "cube" and k in (64, 66))), (name, k, tab[3])
    if (name, k) == ("cornell", 64):
        assert int((tab[0] == 0).sum()) == 10 and tab[3] == 31
    if (name, k) in (("dodge", -70), ("dodge", -66)):
        runs = np.bincount(np.unique(tab[2], return_inverse=True)[1])
        assert tab[3] < sd.ntris - 1 and runs.max() > 2000, "`last` has moved and one threshold repeats thousands of times"


# ---- 6. gradients: the atomic add and subnormals ----
@pytest.fixture(scope="module")
def square(pkg, world):
    sd, sc = world("square", 0)[0:2]
    rays, hits = _square_list(pkg, np.arange(len(PTS)))
    w = _restated(sd, rays, hits)
    assert (w * 16 == np.round(w * 16)).all() and w.min() >= 1 / 16 and w.max() <= 14 / 16, "the precondition of the exactness argument"
    assert _same(_device_weights(sc, rays, hits), w), "the device's weights are these very values"
    return sd, sc


@pytest.mark.parametrize("C", [3, 32])
def test_atomic_add_and_subnormals(pkg, square, monkeypatch, C):
    """Every product is (m / 16) * g with g an integer in [-8, 8] times 2^e: a multiple of 2^(e - 4); with n = 320 items every partial sum
    stays below 2^(e + 16), so under IEEE arithmetic with subnormals kept every order of the additions gives ldexp(the sum at e = 0, e)
    exactly, down to e = -140 (multiples of 2^-144 >= 2^-149).  The header's bound must hold whatever the add does with subnormals; what
    is observed per mapping is printed (an add that flushed an operand or a sum would leave another value at e = -130 and -140), and
    what include/cgrt.h states after the measurement -- subnormals are kept, under every mapping -- is asserted: bit equality at every e."""
    sd, sc = square
    n = 320
    rng = np.random.default_rng(2000 + C)
    rays, hits = _square_list(pkg, _order("shuffled", n, rng))
    w = _restated(sd, rays, hits)
    gi = rng.integers(-8, 9, (n, C))
    inits = (np.zeros((4, C), np.int64), rng.integers(-8, 9, (4, C)))
    d_rays, d_hits = _dev_rays(rays), _dev_hits(hits)
    observed, failures = {}, []
    for e in EXPONENTS:
        g = np.ldexp(gi.astype(np.float64), e).astype(np.float32)
        assert (g.astype(np.float64) == np.ldexp(gi.astype(np.float64), e)).all()
        for ii in inits:
            init = np.ldexp(ii.astype(np.float64), e).astype(np.float32)
            ref0, _, _ = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], gi.astype(np.float32), ii.astype(np.float32))
            ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
            want = np.ldexp(ref0, e)
            # the restatement: float64 holds every partial sum exactly, so ref is the exact sum, and it is a float32
            assert (ref == want).all() and (want.astype(np.float32).astype(np.float64) == want).all() and np.abs(ref0).max() < 2.0 ** 16
            want = want.astype(np.float32)
            if e == -140:
                assert ((want != 0) & (np.abs(want) < sr.FLT_MIN)).sum() >= want.size // 2, "the exact sums are subnormal"
            for mapping in MAPS:
                if mapping is None:
                    monkeypatch.delenv("CGRT_SURFACE_GRAD_MAP", raising=False)
                else:
                    monkeypatch.setenv("CGRT_SURFACE_GRAD_MAP", mapping)
                table = Guarded((4, C))
                table.t.copy_(_dev(init))
                sc.interpolate_hits_grad_tensor(d_rays, d_hits, _dev(g), grad_attr=table.t)
                got = _np(table.t).copy()
                assert table.intact()
                exact = bool((got.view(np.uint32) == want.view(np.uint32)).all())
                observed.setdefault((mapping, e), []).append(exact)
                err, lim = np.abs(got.astype(np.float64) - ref), gr.bound(S, m)
                if not (np.isfinite(got).all() and (err <= lim).all()):
                    failures.append((mapping, e, bool(ii.any()), "beyond the header's bound", float((err / lim).max())))
                if not exact:
                    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                    r, c = bad[0]
                    print(f"C={C} mapping={mapping} e={e} init={'integers' if ii.any() else 'zero'}: {len(bad)} of {got.size} elements are not the "
                          f"exact image; first [{r},{c}] got {float(got[r, c]):.9e} ({got.view(np.uint32)[r, c]:#010x}) want {float(want[r, c]):.9e} "
                          f"({want.view(np.uint32)[r, c]:#010x}); elements that are zero: {int((got == 0).sum())}, in the exact image {int((want == 0).sum())}")
    monkeypatch.delenv("CGRT_SURFACE_GRAD_MAP", raising=False)
    for mapping in MAPS:
        print(f"C={C} mapping={mapping}: exact image at e = " + ", ".join(f"{e}: {all(observed[(mapping, e)])}" for e in EXPONENTS))
    assert not failures, failures
    for mapping in MAPS:  # include/cgrt.h "Order": the hardware add keeps subnormals, under every mapping
        for e in EXPONENTS:
            assert all(observed[(mapping, e)]), (C, mapping, e, "the sum is not the exact image of the sum at e = 0")


# ---- 7. gradients of real items across scale ----
def _capped(sd, prim):
    """hit flags under the counting rule of test_surface_grad_gpu.py::_capped_list: an item becomes a miss where one of its vertices
    would otherwise collect more than M_CAP contributions."""
    tri = np.asarray(sd.tri, np.int64).reshape(-1, 3)
    count = np.zeros(len(np.asarray(sd.pos_nrm).reshape(-1, 6)), np.int64)
    hit = np.ones(len(prim), np.uint32)
    for i, p in enumerate(prim):
        v = tri[p]
        if (count[v] >= gr.M_CAP - 2).any():
            hit[i] = 0
        else:
            np.add.at(count, v, 1)
    return hit


@pytest.mark.parametrize("C", [3, 32])
@pytest.mark.parametrize("k", GRAD_KS)
def test_gradients_of_real_items_across_scale(pkg, world, k, C):
    name = "blob"
    sd, sc, rays, prim, hits = world(name, k)
    hits["hit"] = _capped(sd, prim)
    hits["hit"][7::64] = 0  # misses among the items: their grad_out is never read
    ok = surface_ref.triangle_mask(sd, hits["hit"], hits["prim_id"])
    assert sr.in_surface_envelope(world.measures(name), k).all()
    w = _restated(sd, rays, hits)
    sd0, _, rays0, _, hits0 = world(name, 0)
    hits0["hit"] = hits["hit"]
    assert _same(w, _restated(sd0, rays0, hits0)), "inside the envelope the restated weights are those of scale 1: so is the expected gradient"
    rng = np.random.default_rng(C)
    g = _values(rng, (N, C))
    g[~ok] = np.nan
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    init = _values(rng, (nverts, C))
    ref, S, m = gr.adjoint(sd, w, hits["prim_id"], hits["hit"], g, init)
    assert m.max() <= gr.M_CAP and (m > 0).sum() > 100
    table = Guarded(init.shape)
    table.t.copy_(_dev(init))
    sc.interpolate_hits_grad_tensor(_dev_rays(rays), _dev_hits(hits), _dev(g), grad_attr=table.t)
    got = _np(table.t)
    beyond, touched = gr.check(got, ref, S, m, f"{name} 2^{k} C={C}")
    assert touched > 0 and beyond == 0
    assert np.array_equal(got[m == 0].view(np.uint32), init[m == 0].view(np.uint32)), "rows no valid item names keep their bytes"
    assert table.intact()

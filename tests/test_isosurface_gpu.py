"""GPU: iso-surfaces (cgrt_isosurface*; include/cgrt.h "Iso-surfaces").  Every comparison is byte for byte against the
numpy restatement tests/isosurface_ref.py, whose table is derived by rule.

* Dims (2,2,2), (3,2,2), (1,5,5) and (2,1,2) (both empty), (17,9,5) and (65,33,4) (block and row straddles), (96,64,64) (1 536 blocks: more
  than one scan tile); fields sphere, torus, gyroid, uniform noise at iso 0 (every cell crossed), a constant (empty), the integer field
  with values equal to iso, noise with 1 % NaN and +-inf, iso above the maximum and below the minimum; both flags.
* Per case: the count form equals the list form's counts; capacities (0, 0), (1, 1), exact and exact - 1 with guard bytes around verts,
  tris, counts and the workspace (which sits 8 bytes off a 16-byte boundary, filled with 0xA5); the host form; the four work counters.
* A workspace one byte short is CGRT_E_ARG with nothing written; four host threads and a side stream give the same bytes; the prediction
  record, the hint state and the layout hash do not move; both scale symmetries.
* End to end: the cube's offset surface (sdf_isosurface_tensor) is closed, equals the restatement on the same values, and wrapped by
  mesh_scene_data into a Scene has winding number +-1 / 0 on the right side of every grid point away from the level; the monkey's (open)
  winding stand-in is closed."""
import threading

import numpy as np
import pytest

import isosurface_ref as iref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
DIMS = ((2, 2, 2), (3, 2, 2), (1, 5, 5), (2, 1, 2), (17, 9, 5), (65, 33, 4), (96, 64, 64))
BIG = (96, 64, 64)
FIELDS = ("sphere", "torus", "gyroid", "noise", "constant")
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")


@pytest.fixture(scope="module")
def sc(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=0)
    yield s
    s.close()


_refs = {}


def _case(name, dims, iso=0.0, above=False):
    """(values, origin, spacing, (verts, tris, work)) of a named field: computed once, shared by the tests, never changed."""
    key = (name, tuple(dims), float(iso), bool(above))
    if key not in _refs:
        if name == "integer":
            val, o, sp = iref.integer_field()
        elif name == "nonfinite":
            val, o, sp = iref.field("noise", dims, seed=3)
            rng = np.random.default_rng(11)
            flat = val.reshape(-1)
            bad = rng.random(flat.size) < 0.01
            flat[bad] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), int(bad.sum()))
        else:
            val, o, sp = iref.field(name, dims, box=1.6 if name == "torus" else 1.2, seed=1)
        ref = iref.isosurface(val, o, sp, iso=iso, inside_above=above, want_work=True)
        for a in (val, o, sp, ref[0], ref[1]):
            a.setflags(write=False)
        _refs[key] = (val, o, sp, ref)
    return _refs[key]


class Guarded:
    """nbytes of device memory between two guards, all of it 0xA5 before the call; `shift` moves it off 16-byte alignment."""

    def __init__(self, nbytes, shift=0):
        self.n, self.lo = int(nbytes), PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def bytes(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[self.lo : self.lo + self.n]

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[: self.lo] == SENTINEL).all() and (b[self.lo + self.n :] == SENTINEL).all())


def _device(sc, val, o, sp, iso, above, vcap, tcap, stream=None, tv=None):
    """cgrt_isosurface_device with guards: (the vertex array's bytes, the triangle array's bytes, counts)."""
    dims = val.shape[::-1]
    tv = torch.from_numpy(np.ascontiguousarray(val).copy()).cuda() if tv is None else tv
    nbytes = sc.isosurface_workspace(dims)
    verts, tris, counts, ws = Guarded(12 * vcap), Guarded(12 * tcap), Guarded(16), Guarded(nbytes, shift=8)
    assert ws.ptr() % 16 == 8
    torch.cuda.synchronize()
    sc.isosurface_device(o, sp, dims, tv.data_ptr(), verts.ptr() if vcap else 0, vcap, tris.ptr() if tcap else 0, tcap, counts.ptr(), ws.ptr(),
                         nbytes, iso=iso, inside_above=above, stream=(stream or torch.cuda.current_stream()).cuda_stream)
    assert verts.intact() and tris.intact() and counts.intact() and ws.intact(), ("guards", dims, vcap, tcap)
    return verts.bytes(), tris.bytes(), tuple(int(x) for x in counts.bytes().view(np.uint64))


def _count(sc, val, o, sp, iso, above, tv=None):
    dims = val.shape[::-1]
    tv = torch.from_numpy(np.ascontiguousarray(val).copy()).cuda() if tv is None else tv
    nbytes = sc.isosurface_workspace(dims)
    counts, ws = Guarded(16), Guarded(nbytes, shift=8)
    sc.isosurface_count_device(o, sp, dims, tv.data_ptr(), counts.ptr(), ws.ptr(), nbytes, iso=iso, inside_above=above)
    assert counts.intact() and ws.intact()
    return tuple(int(x) for x in counts.bytes().view(np.uint64))


def _expect(got, want, what):
    """got: the bytes of a guarded array of some capacity; want: the restatement's full array"""
    rows = len(got) // 12
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    k = min(rows, len(want))
    if not np.array_equal(got[: 12 * k], w[: 12 * k]):
        g, ww = got[: 12 * k].view(np.uint32).reshape(-1, 3), w[: 12 * k].view(np.uint32).reshape(-1, 3)
        bad = np.flatnonzero((g != ww).any(1))
        raise AssertionError(f"{what}: {len(bad)} of {k} rows differ, first at {bad[0]}: {g[bad[0]]} != {ww[bad[0]]}")
    assert (got[12 * k :] == SENTINEL).all(), f"{what}: a row beyond the count was written"


def _check(sc, val, o, sp, ref, iso=0.0, above=False, host=True):
    """Every form against the restatement's (verts, tris, work)."""
    verts, tris, work = ref
    nv, nt = len(verts), len(tris)
    tv = torch.from_numpy(np.ascontiguousarray(val).copy()).cuda()
    assert _count(sc, val, o, sp, iso, above, tv) == (nv, nt), "count form"
    for vcap, tcap in {(0, 0), (1, 1), (nv, nt), (max(nv - 1, 0), max(nt - 1, 0))}:
        gv, gt, counts = _device(sc, val, o, sp, iso, above, vcap, tcap, tv=tv)
        assert counts == (nv, nt), ("the counts are the full counts whatever the capacities", vcap, tcap)
        _expect(gv, verts, ("verts", vcap, tcap))
        _expect(gt, tris, ("tris", vcap, tcap))
    if host:
        hv, ht = sc.isosurface(val, o, sp, iso=iso, inside_above=above)
        assert hv.shape == verts.shape and ht.shape == tris.shape and hv.tobytes() == verts.tobytes() and ht.tobytes() == tris.tobytes(), "host form"
        assert sc.debug_isosurface_work(val, o, sp, iso=iso, inside_above=above) == work


# ---- dims x fields ----
@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_dims_and_fields(sc, dims, name):
    val, o, sp, ref = _case(name, dims)
    if min(dims) < 2 or name == "constant":
        assert len(ref[0]) == 0 and len(ref[1]) == 0
    elif name == "noise":
        cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
        # (eight corners of one sign: 2 cells in 256)
        assert ref[2][0] >= 0.95 * cells or cells < 64, "uniform noise crosses all but 1 cell in 128: the densest counts"
    _check(sc, val, o, sp, ref)
    if dims != BIG:
        val, o, sp, ref = _case(name, dims, iso=0.125, above=True)
        _check(sc, val, o, sp, ref, iso=0.125, above=True)


def test_big_grid_facing_the_other_way(sc):
    val, o, sp, ref = _case("gyroid", BIG, above=True)
    _check(sc, val, o, sp, ref, above=True, host=False)
    fwd = _case("gyroid", BIG)[3]
    assert ref[0].tobytes() == fwd[0].tobytes() and ref[1].tobytes() != fwd[1].tobytes() and len(ref[1]) == len(fwd[1])


@pytest.mark.parametrize("above", [False, True])
def test_values_equal_to_iso(sc, above):
    val, o, sp, ref = _case("integer", (7, 7, 7), above=above)
    if not above:
        assert (len(ref[0]), len(ref[1])) == (74, 144) and iref.is_closed(ref[1])
    assert (val == 0).sum() > 0
    _check(sc, val, o, sp, ref, above=above)


@pytest.mark.parametrize("dims", [(17, 9, 5), (65, 33, 4), BIG], ids=lambda d: "x".join(map(str, d)))
def test_non_finite_values(sc, dims):
    val, o, sp, ref = _case("nonfinite", dims)
    assert np.isnan(val).any() and np.isposinf(val).any() and np.isneginf(val).any()
    assert 0 < ref[2][0] < (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    _check(sc, val, o, sp, ref)
    if dims != BIG:
        val, o, sp, ref = _case("nonfinite", dims, above=True)
        _check(sc, val, o, sp, ref, above=True)


@pytest.mark.parametrize("iso", [5.0, -5.0])
@pytest.mark.parametrize("above", [False, True])
def test_iso_outside_the_range(sc, iso, above):
    val, o, sp, ref = _case("noise", (17, 9, 5), iso=iso, above=above)
    assert val.min() > -5.0 and val.max() < 5.0 and len(ref[0]) == 0 and len(ref[1]) == 0
    _check(sc, val, o, sp, ref, iso=iso, above=above)


# ---- the workspace, threads, streams ----
def test_a_short_workspace_is_refused_with_nothing_written(pkg, sc):
    val, o, sp, ref = _case("sphere", (17, 9, 5))
    dims = val.shape[::-1]
    tv = torch.from_numpy(val.copy()).cuda()
    nbytes = sc.isosurface_workspace(dims)
    verts, tris, counts, ws = Guarded(12 * len(ref[0])), Guarded(12 * len(ref[1])), Guarded(16), Guarded(nbytes, shift=8)
    for kw in (dict(d_workspace_ptr=ws.ptr(), workspace_bytes=nbytes - 1), dict(d_workspace_ptr=ws.ptr() + 4, workspace_bytes=nbytes),
               dict(d_workspace_ptr=0, workspace_bytes=nbytes)):
        with pytest.raises(pkg.CgrtError) as e:
            sc.isosurface_device(o, sp, dims, tv.data_ptr(), verts.ptr(), len(ref[0]), tris.ptr(), len(ref[1]), counts.ptr(), **kw)
        assert e.value.code == -1, kw
        with pytest.raises(pkg.CgrtError) as e:
            sc.isosurface_count_device(o, sp, dims, tv.data_ptr(), counts.ptr(), **kw)
        assert e.value.code == -1, kw
    # a workspace that is large enough by its argument but not device memory: refused by the span check, before any work
    host = np.zeros(nbytes + 16, np.uint8)
    with pytest.raises(pkg.CgrtError) as e:
        sc.isosurface_device(o, sp, dims, tv.data_ptr(), verts.ptr(), len(ref[0]), tris.ptr(), len(ref[1]), counts.ptr(),
                             host.ctypes.data + (-host.ctypes.data) % 8, nbytes)
    assert e.value.code == -1
    for g in (verts, tris, counts, ws):
        assert (g.bytes() == SENTINEL).all() and g.intact(), "refused before any work"
    assert not host.any()


def test_four_threads_and_a_side_stream(sc):
    jobs = [_case("sphere", (17, 9, 5)), _case("noise", (65, 33, 4)), _case("gyroid", (65, 33, 4)), _case("torus", (17, 9, 5))]
    tvs = [torch.from_numpy(j[0].copy()).cuda() for j in jobs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    results, errors = {}, []

    def work(t):
        try:
            s = streams[t]
            for it in range(3):
                k = (t + it) % len(jobs)
                val, o, sp, ref = jobs[k]
                with torch.cuda.stream(s):
                    res = sc.isosurface_tensor(tvs[k], o, sp, stream=s)
                    s.synchronize()
                results[(t, it)] = (k, res["verts"].cpu().numpy(), res["tris"].cpu().numpy(), sc.isosurface(val, o, sp))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 12
    for (t, it), (k, dv, dt, (hv, ht)) in results.items():
        verts, tris, _ = jobs[k][3]
        assert dv.tobytes() == verts.tobytes() and dt.tobytes() == tris.tobytes(), ("device, threaded", t, it)
        assert hv.tobytes() == verts.tobytes() and ht.tobytes() == tris.tobytes(), ("host, threaded", t, it)
    side = torch.cuda.Stream()
    val, o, sp, ref = jobs[1]
    gv, gt, counts = _device(sc, val, o, sp, 0.0, False, len(ref[0]), len(ref[1]), stream=side)
    assert counts == (len(ref[0]), len(ref[1]))
    _expect(gv, ref[0], "verts, side stream")
    _expect(gt, ref[1], "tris, side stream")


def test_tensor_forms(sc):
    val, o, sp, ref = _case("gyroid", (65, 33, 4))
    verts, tris, _ = ref
    tv = torch.from_numpy(val.copy()).cuda()
    res = sc.isosurface_tensor(tv, o, sp)
    assert res["verts"].dtype == torch.float32 and res["tris"].dtype == torch.int32 and res["counts"].dtype == torch.int64
    assert tuple(res["counts"].cpu().numpy()) == (len(verts), len(tris))
    assert res["verts"].cpu().numpy().tobytes() == verts.tobytes() and res["tris"].cpu().numpy().tobytes() == tris.tobytes()
    ws = torch.zeros(sc.isosurface_workspace(val.shape[::-1]) + 8, dtype=torch.uint8, device="cuda")
    over = sc.isosurface_tensor(tv, o, sp, capacity=(len(verts) + 100, len(tris) + 7), workspace=ws)
    assert over["verts"].shape == (len(verts), 3) and over["tris"].shape == (len(tris), 3)
    assert over["verts"].cpu().numpy().tobytes() == verts.tobytes() and over["tris"].cpu().numpy().tobytes() == tris.tobytes()
    under = sc.isosurface_tensor(tv, o, sp, capacity=(10, 5))
    assert tuple(under["counts"].cpu().numpy()) == (len(verts), len(tris))
    assert under["verts"].cpu().numpy().tobytes() == verts[:10].tobytes() and under["tris"].cpu().numpy().tobytes() == tris[:5].tobytes()
    with pytest.raises(ValueError):
        sc.isosurface_tensor(tv.reshape(-1), o, sp)
    with pytest.raises(ValueError):
        sc.isosurface_tensor(tv, o, sp, workspace=ws[:100])


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
        base = a.device_bytes()
        val, o, sp, ref = _case("sphere", (17, 9, 5))
        a.isosurface(val, o, sp)
        a.debug_isosurface_work(val, o, sp)
        a.isosurface_tensor(torch.from_numpy(val.copy()).cuda(), o, sp)
        torch.cuda.synchronize()
        assert a.device_bytes() == base, "no table is made or uploaded"
        for _ in range(3):
            ref_b = b.render(cam, W, H)
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref_b[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("k", [-20, 20])
def test_scale_symmetries(sc, k):
    val, o, sp, ref = _case("gyroid", (17, 9, 5), iso=0.0625)
    verts, tris, _ = ref
    s = np.float32(2.0**k)
    v1, t1 = sc.isosurface(val, o * s, sp * s, iso=0.0625)
    assert v1.tobytes() == (verts * s).tobytes() and t1.tobytes() == tris.tobytes() and len(tris) > 0
    v2, t2 = sc.isosurface(val * s, o, sp, iso=float(np.float32(0.0625) * s))
    assert v2.tobytes() == verts.tobytes() and t2.tobytes() == tris.tobytes()
    tv = torch.from_numpy(val * s).cuda()
    res = sc.isosurface_tensor(tv, o, sp, iso=float(np.float32(0.0625) * s))
    assert res["verts"].cpu().numpy().tobytes() == verts.tobytes() and res["tris"].cpu().numpy().tobytes() == tris.tobytes()


# ---- end to end ----
def _fixture_grid(sd, n, margin):
    p = np.asarray(sd.pos_nrm, np.float32)[:, :3].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    ext = float((hi - lo).max())
    origin = (lo - margin * ext).astype(np.float32)
    spacing = ((hi - lo + 2.0 * margin * ext) / (n - 1)).astype(np.float32)
    return origin, spacing, ext


def test_cube_offset_surface_end_to_end(pkg, scene_data):
    sd = scene_data("cube")
    n = 24
    origin, spacing, ext = _fixture_grid(sd, n, 0.5)
    offset = float(np.float32(0.1 * ext))
    src = pkg.Scene(sd, device=0)
    try:
        res = src.sdf_isosurface_tensor(origin, spacing, (n, n, n), offset=offset)
        val = res["values"].cpu().numpy()
        verts, tris = res["verts"].cpu().numpy(), res["tris"].cpu().numpy().view(np.uint32)
        rv, rt = iref.isosurface(val, origin, spacing, iso=offset)
        assert verts.tobytes() == rv.tobytes() and tris.tobytes() == rt.tobytes() and len(rt) > 0
        assert iref.is_closed(tris) and iref.unreferenced(len(verts), tris) == 0 and iref.signed_volume(verts, tris) > 0
        flip = src.isosurface_tensor(-res["values"], origin, spacing, iso=-offset, inside_above=True)
        fv, ft = flip["verts"].cpu().numpy(), flip["tris"].cpu().numpy().view(np.uint32)
        assert fv.tobytes() == verts.tobytes() and ft.tobytes() == tris.tobytes()
        back = src.isosurface_tensor(res["values"], origin, spacing, iso=offset, inside_above=True)
        bt = back["tris"].cpu().numpy().view(np.uint32)
        assert back["verts"].cpu().numpy().tobytes() == verts.tobytes() and iref.is_closed(bt)
    finally:
        src.close()
    # every grid point at least two spacings' worth of distance from the level is at least 0.27 spacings from any crossed cell (the SDF
    # is 1-Lipschitz and a cell's diagonal is sqrt(3) spacings): its winding number is decided
    pts = pkg.sdf_grid_points(origin, spacing, (n, n, n))
    far = np.abs(val.reshape(-1) - np.float32(offset)) > 2.0 * float(spacing.max())
    inside = (val.reshape(-1) < np.float32(offset))[far]
    assert inside.sum() > 100 and (~inside).sum() > 100
    signs = []
    for t in (tris, bt):
        new = pkg.Scene(pkg.scenes.mesh_scene_data(verts, t), device=0)
        try:
            w = new.winding_numbers_brute(pts[far], want="w")
        finally:
            new.close()
        sign = np.sign(w[inside][0])
        print(f"winding numbers: inside |w - {sign:+.0f}| <= {np.abs(w[inside] - sign).max():.2e}, outside |w| <= {np.abs(w[~inside]).max():.2e}")
        assert sign != 0 and (np.abs(w[inside] - sign) < 0.01).all() and (np.abs(w[~inside]) < 0.01).all()
        signs.append(sign)
    assert signs[0] == -signs[1], "the triangles face the other way under inside_above"


def test_monkey_winding_stand_in_is_closed(pkg, scene_data):
    sd = scene_data("monkey")
    n = 32
    origin, spacing, _ = _fixture_grid(sd, n, 0.25)
    src = pkg.Scene(sd, device=0)
    try:
        res = src.winding_isosurface_tensor(origin, spacing, (n, n, n))
        val = res["values"].cpu().numpy()
        verts, tris = res["verts"].cpu().numpy(), res["tris"].cpu().numpy().view(np.uint32)
    finally:
        src.close()
    boundary = np.ones(val.shape, bool)
    boundary[1:-1, 1:-1, 1:-1] = False
    assert (val[boundary] < 0.5).all(), "the margin keeps the level off the grid's boundary"
    assert len(tris) > 1000 and iref.is_closed(tris) and iref.unreferenced(len(verts), tris) == 0
    rv, rt = iref.isosurface(val, origin, spacing, iso=0.5, inside_above=True)
    assert verts.tobytes() == rv.tobytes() and tris.tobytes() == rt.tobytes()
    assert iref.signed_volume(verts, tris) > 0

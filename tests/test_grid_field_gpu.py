"""GPU: grid fields (cgrt_sample_grid*, cgrt_march_grid*; include/cgrt.h "Grid fields").  Every comparison is byte for
byte against the numpy restatement tests/grid_field_ref.py.

* Sampling: dims (2,2,2), (3,2,2), (17,9,5), (65,33,4), (96,64,64); fields sphere, noise, integer, noise with 1 % NaN and +-inf; n in
  {1, 63, 64, 65, 4 099}; points on grid points, on faces, outside, NaN and inf; both flags; each subset of the outputs; guard bytes
  (0xA5) around every output, all of them 4 bytes off a 16-byte boundary.
* Marching: n in {1, 65, 4 096}; the three parameter sets of the CPU file, max_steps 1 and 7, a finite t_ray; the sphere and the
  non-finite field; the records and the three work counters.
* The host form equals the device form; four host threads and a side stream give the same bytes; the prediction record, the hint state
  and the layout hash do not move.
* End to end: the cube's signed distances on 33^3, marched at 0.25 of its extent by 4 096 camera rays."""
import itertools
import threading

import numpy as np
import pytest

import grid_field_ref as gref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
SENTINEL = 0xA5
PAD = 256
DIMS = ((2, 2, 2), (3, 2, 2), (17, 9, 5), (65, 33, 4), (96, 64, 64))
FIELDS = ("sphere", "noise", "integer", "nonfinite")
COUNTS = (1, 63, 64, 65, 4099)
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")
PAYLOAD = np.asarray([0x7FC00ABC], np.uint32).view(F)[0]
MARCH_SETS = {
    "sphere-trace": dict(relax=1.0, min_step=1e-4, hit_eps=1e-4, max_steps=256),
    "half-relaxed": dict(relax=0.5, min_step=1e-4, hit_eps=1e-4, max_steps=256),
    "fixed-refined": dict(relax=0.0, min_step=0.01, hit_eps=1e-4, max_steps=1024, refine=16),
    "one-step": dict(relax=1.0, min_step=1e-4, hit_eps=1e-4, max_steps=1),
    "seven-steps": dict(relax=0.0, min_step=0.05, hit_eps=1e-4, max_steps=7, refine=3),
}


@pytest.fixture(scope="module")
def sc(pkg, scene_data):
    s = pkg.Scene(scene_data("cube"), device=0)
    yield s
    s.close()


_fields, _points, _rays = {}, {}, {}


def _field(name, dims):
    """(values (nz, ny, nx), origin, spacing) on [-1.2, 1.2]^3, the y axis running backwards: made once, never changed."""
    key = (name, tuple(dims))
    if key not in _fields:
        nx, ny, nz = dims
        sp = np.asarray([2.4 / (nx - 1), -2.4 / (ny - 1), 2.4 / (nz - 1)], F)
        o = np.asarray([-1.2, 1.2, -1.2], F)
        ax = [o[c].astype(np.float64) + np.arange(n) * float(sp[c]) for c, n in enumerate(dims)]
        X, Y, Z = ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None]
        rng = np.random.default_rng(1)
        if name == "sphere":
            val = np.sqrt(X * X + Y * Y + Z * Z) - 0.8
        elif name == "integer":
            val = np.abs(np.arange(nx) - nx // 2)[None, None, :] + np.abs(np.arange(ny) - ny // 2)[None, :, None] * 2.0 + \
                np.abs(np.arange(nz) - nz // 2)[:, None, None] * 4.0 - 2.0
        else:
            val = rng.uniform(-1, 1, size=(nz, ny, nx))
        val = np.ascontiguousarray(np.broadcast_to(val, (nz, ny, nx)), F).copy()
        if name == "nonfinite":
            flat = val.reshape(-1)
            bad = rng.random(flat.size) < 0.01
            bad[0] = True
            flat[bad] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], F), int(bad.sum()))
        for a in (val, o, sp):
            a.setflags(write=False)
        _fields[key] = (val, o, sp)
    return _fields[key]


def _mixed_points(dims, o, sp, n):
    """n points: grid points, face points, points inside, points outside, NaN and inf points."""
    key = (tuple(dims), n)
    if key not in _points:
        rng = np.random.default_rng(n)
        top = (np.asarray(dims) - 1).astype(np.float64)
        kind = np.arange(n) % 8
        u = rng.uniform(0, 1, size=(n, 3)) * top
        grid = np.floor(rng.uniform(0, 1, size=(n, 3)) * (top + 1))
        u = np.where((kind == 0)[:, None], grid, u)  # grid points, the last planes included
        face = kind == 1  # on a face of the box: one coordinate at 0 or at the top
        axis = rng.integers(0, 3, n)
        side = rng.integers(0, 2, n)
        for c in range(3):
            u[:, c] = np.where(face & (axis == c), side * top[c], u[:, c])
        u = np.where((kind == 2)[:, None], rng.uniform(-0.5, 1.5, size=(n, 3)) * top, u)  # many of them outside
        p = (o.astype(np.float64) + u * sp.astype(np.float64)).astype(F)
        p[kind == 0] = (o + grid[kind == 0].astype(F) * sp).astype(F)  # exactly as the grid makes them
        odd = np.asarray([np.nan, np.inf, -np.inf], F)
        rows = np.flatnonzero(kind == 3)
        p[rows, rng.integers(0, 3, len(rows))] = odd[rng.integers(0, 3, len(rows))]
        p.setflags(write=False)
        _points[key] = p
    return _points[key]


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


def _misaligned(a):
    """A device copy of a float32 array that starts 4 bytes off a 16-byte boundary."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    g = Guarded(len(raw), shift=4)
    g.buf[g.lo : g.lo + g.n] = torch.from_numpy(raw.copy()).cuda()
    assert g.ptr() % 16 == 4
    return g


SUBSETS = [s for k in (1, 2, 3) for s in itertools.combinations(("value", "gradient", "inside"), k)]


@pytest.mark.parametrize("name", FIELDS)
@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
def test_sampling(sc, dims, name):
    val, o, sp = _field(name, dims)
    tv = _misaligned(val)
    for n in COUNTS:
        p = _mixed_points(dims, o, sp, n)
        tp = _misaligned(p)
        for clamp in (False, True):
            vw, gw, ins = gref.sample(val, o, sp, p, outside=PAYLOAD, clamp=clamp)
            want = {"value": vw.tobytes(), "gradient": gw.tobytes(), "inside": ins.tobytes()}
            # every subset of the outputs at one size, all three at the others
            for subset in (SUBSETS if n == 65 else [("value", "gradient", "inside")]):
                out = {w: Guarded({"value": 4, "gradient": 12, "inside": 1}[w] * n, shift=4) for w in subset}
                sc.sample_grid_device(o, sp, dims, tv.ptr(), tp.ptr(), n, *(out[w].ptr() if w in out else 0 for w in ("value", "gradient", "inside")),
                                      outside=PAYLOAD, clamp=clamp)
                for w in subset:
                    assert out[w].intact(), ("guards", w, n, clamp, subset)
                    assert out[w].bytes().tobytes() == want[w], (w, n, clamp, subset)
        assert tv.intact() and tp.intact()
    # the host form, and NULL parameters ({NaN, 0})
    p = _mixed_points(dims, o, sp, 4099)
    vw, gw, ins = gref.sample(val, o, sp, p, outside=PAYLOAD, clamp=True)
    res = sc.sample_grid(val, o, sp, p, outside=PAYLOAD, clamp=True)
    assert res["value"].tobytes() == vw.tobytes() and res["gradient"].tobytes() == gw.tobytes() and res["inside"].tobytes() == ins.tobytes()
    vw, gw, ins = gref.sample(val, o, sp, p[:65])
    res = sc.sample_grid(val, o, sp, p[:65], want=("value", "inside"))
    assert set(res) == {"value", "inside"} and res["value"].tobytes() == vw.tobytes() and res["inside"].tobytes() == ins.tobytes()


def test_sampling_tensor_form(sc):
    dims = (17, 9, 5)
    val, o, sp = _field("noise", dims)
    p = _mixed_points(dims, o, sp, 4099)
    vw, gw, ins = gref.sample(val, o, sp, p, outside=0.0)
    tv, tp = torch.from_numpy(val.copy()).cuda(), torch.from_numpy(p.copy()).cuda()
    res = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0)
    assert res["value"].dtype == torch.float32 and res["gradient"].shape == (4099, 3) and res["inside"].dtype == torch.bool
    assert res["value"].cpu().numpy().tobytes() == vw.tobytes() and res["gradient"].cpu().numpy().tobytes() == gw.tobytes()
    assert res["inside"].cpu().numpy().view(np.uint8).tobytes() == ins.tobytes()
    mine = torch.zeros((4099, 3), dtype=torch.float32, device="cuda")
    res = sc.sample_grid_tensor(tv, o, sp, tp, outside=0.0, want="gradient", out={"gradient": mine})
    assert set(res) == {"gradient"} and res["gradient"] is mine and mine.cpu().numpy().tobytes() == gw.tobytes()
    assert sc.sample_grid_tensor(tv, o, sp, tp[:0])["value"].shape == (0,)
    with pytest.raises(ValueError):
        sc.sample_grid_tensor(tv.reshape(-1), o, sp, tp)
    with pytest.raises(ValueError):
        sc.sample_grid_tensor(tv, o, sp, tp, want=("value", "colour"))


# ---- marching ----
def _march_rays(n, normalised, finite_t):
    key = (n, normalised, finite_t)
    if key not in _rays:
        rng = np.random.default_rng(7)
        o = rng.standard_normal((n, 3))
        o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
        d = rng.standard_normal((n, 3)) - o
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        if not normalised:
            d = d * rng.uniform(0.5, 2.0, size=(n, 1))
        r = np.zeros((n, 7), F)
        r[:, 0:3], r[:, 3:6], r[:, 6] = o, d, np.finfo(F).max
        if finite_t:
            r[:, 6] = rng.uniform(0.0, 5.0, n)
        if n > 8:  # rays of every other kind: axis-parallel, zero, non-finite, starting inside the level
            r[1, 3:6] = (0, 0, 1)
            r[2, 0:6] = (0.1, 0.2, -3, 0, 0, 2)
            r[3, 3:6] = 0
            r[4, 0] = np.nan
            r[5, 5] = np.inf
            r[6, 6] = np.nan
            r[7, 0:3] = (0.1, 0.1, 0.1)
        r.setflags(write=False)
        _rays[key] = r
    return _rays[key]


def _marched(name, dims, rays_key, set_name):
    key = (name, dims, rays_key, set_name)
    if key not in _marched_cache:
        val, o, sp = _field(name, dims)
        _marched_cache[key] = gref.march(val, o, sp, _march_rays(*rays_key), iso=0.0, **MARCH_SETS[set_name])
    return _marched_cache[key]


_marched_cache = {}


@pytest.mark.parametrize("set_name", list(MARCH_SETS))
@pytest.mark.parametrize("name", ["sphere", "nonfinite"])
def test_marching(sc, name, set_name):
    dims = (33, 33, 33) if name == "sphere" else (17, 9, 5)
    val, o, sp = _field(name, dims)
    tv = _misaligned(val)
    prm = MARCH_SETS[set_name]
    statuses = set()
    for n, finite_t in ((1, False), (65, False), (4096, False), (4096, True)):
        rays_key = (n, set_name == "fixed-refined", finite_t)
        rays = _march_rays(*rays_key)
        rec, work = _marched(name, dims, rays_key, set_name)
        tr, hits = _misaligned(rays), Guarded(32 * n, shift=4)
        sc.march_grid_device(o, sp, dims, tv.ptr(), tr.ptr(), n, hits.ptr(), iso=0.0, **prm)
        assert hits.intact() and tr.intact(), ("guards", n, finite_t)
        got = hits.bytes().view(gref.HIT_DTYPE)
        if got.tobytes() != rec.tobytes():
            bad = np.flatnonzero(got.view(np.uint32).reshape(-1, 8) != rec.view(np.uint32).reshape(-1, 8))
            raise AssertionError(f"{n} rays, finite t {finite_t}: record {bad[0] // 8} differs: {got[bad[0] // 8]} != {rec[bad[0] // 8]}")
        if n in (65, 4096) and not finite_t:
            assert sc.debug_march_work(val, o, sp, rays, iso=0.0, **prm) == work, ("work", n)
        statuses |= set(int(x) for x in rec["status"])
    assert tv.intact()
    assert {gref.MISS} < statuses, "the case covers more than misses"
    if name == "nonfinite":
        assert gref.NONFINITE in statuses
    if set_name in ("one-step", "seven-steps"):
        assert gref.EXHAUSTED in statuses


def test_marching_inside_above(sc):
    dims = (33, 33, 33)
    val, o, sp = _field("sphere", dims)
    rays = _march_rays(4096, False, False)
    prm = dict(MARCH_SETS["sphere-trace"], refine=5)
    rec, _ = gref.march(-val, o, sp, rays, iso=0.0, inside_above=True, **prm)
    got = sc.march_grid(-val, o, sp, rays, iso=0.0, inside_above=True, **prm)
    assert got.tobytes() == rec.tobytes() and (rec["status"] == gref.HIT).sum() > 500


def test_host_form_and_tensor_form(sc):
    dims = (33, 33, 33)
    val, o, sp = _field("sphere", dims)
    rays_key = (4096, False, False)
    rays = _march_rays(*rays_key)
    rec, _ = _marched("sphere", dims, rays_key, "sphere-trace")
    prm = MARCH_SETS["sphere-trace"]
    assert sc.march_grid(val, o, sp, rays, iso=0.0, **prm).tobytes() == rec.tobytes()
    assert sc.march_grid(val, o, sp, rays[:0], iso=0.0, **prm).shape == (0,)
    tv, tr = torch.from_numpy(val.copy()).cuda(), torch.from_numpy(rays.copy()).cuda()
    res = sc.march_grid_tensor(tv, o, sp, tr, iso=0.0, **prm)
    assert res["records"].shape == (4096, 8) and res["records"].cpu().numpy().tobytes() == rec.tobytes()
    assert res["t"].cpu().numpy().tobytes() == rec["t"].tobytes() and res["value"].cpu().numpy().tobytes() == rec["value"].tobytes()
    assert res["steps"].dtype == torch.int32 and np.array_equal(res["steps"].cpu().numpy(), rec["steps"].astype(np.int32))
    assert np.array_equal(res["status"].cpu().numpy(), rec["status"].astype(np.int32))
    assert res["gradient"].shape == (4096, 3) and res["gradient"].cpu().numpy().tobytes() == rec["gradient"].tobytes()
    for k in ("t", "value", "steps", "status", "gradient"):
        assert res[k].untyped_storage().data_ptr() == res["records"].untyped_storage().data_ptr(), "views over one tensor"
    with pytest.raises(ValueError):
        sc.march_grid_tensor(tv, o, sp, tr.reshape(-1), iso=0.0, **prm)


def test_refused_before_any_work(pkg, sc):
    dims = (17, 9, 5)
    val, o, sp = _field("noise", dims)
    tv, tr, hits = _misaligned(val), _misaligned(_march_rays(65, False, False)), Guarded(32 * 65, shift=4)
    host = np.zeros(32 * 65 + 16, np.uint8)
    for kw in (dict(d_hits_ptr=hits.ptr() + 2), dict(d_hits_ptr=host.ctypes.data + (-host.ctypes.data) % 4), dict(d_hits_ptr=hits.ptr(), max_steps=0)):
        with pytest.raises(pkg.CgrtError) as e:
            sc.march_grid_device(o, sp, dims, tv.ptr(), tr.ptr(), 65, **dict(dict(iso=0.0), **kw))
        assert e.value.code == -1, kw
    assert (hits.bytes() == SENTINEL).all() and hits.intact() and not host.any()


def test_four_threads_and_a_side_stream(sc):
    dims = (33, 33, 33)
    val, o, sp = _field("sphere", dims)
    names = ["sphere-trace", "half-relaxed", "fixed-refined", "seven-steps"]
    keys = [(4096, nm == "fixed-refined", False) for nm in names]
    refs = [_marched("sphere", dims, k, nm)[0] for k, nm in zip(keys, names)]
    p = _mixed_points(dims, o, sp, 4099)
    sample_ref = gref.sample(val, o, sp, p, outside=PAYLOAD)
    tv, tp = torch.from_numpy(val.copy()).cuda(), torch.from_numpy(p.copy()).cuda()
    trs = [torch.from_numpy(_march_rays(*k).copy()).cuda() for k in keys]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(4)]
    results, errors = {}, []

    def work(t):
        try:
            s = streams[t]
            for it in range(3):
                k = (t + it) % 4
                with torch.cuda.stream(s):
                    dev = sc.march_grid_tensor(tv, o, sp, trs[k], stream=s, iso=0.0, **MARCH_SETS[names[k]])["records"]
                    smp = sc.sample_grid_tensor(tv, o, sp, tp, outside=PAYLOAD, stream=s)
                    s.synchronize()
                host = sc.march_grid(val, o, sp, _march_rays(*keys[k]), iso=0.0, **MARCH_SETS[names[k]])
                results[(t, it)] = (k, dev.cpu().numpy(), host, smp["value"].cpu().numpy(), smp["gradient"].cpu().numpy())
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(results) == 12
    for (t, it), (k, dev, host, sv, sg) in results.items():
        assert dev.tobytes() == refs[k].tobytes(), ("device, threaded", t, it)
        assert host.tobytes() == refs[k].tobytes(), ("host, threaded", t, it)
        assert sv.tobytes() == sample_ref[0].tobytes() and sg.tobytes() == sample_ref[1].tobytes(), ("samples, threaded", t, it)
    side = torch.cuda.Stream()
    hits = Guarded(32 * 4096, shift=4)
    torch.cuda.synchronize()
    sc.march_grid_device(o, sp, dims, tv.data_ptr(), trs[0].data_ptr(), 4096, hits.ptr(), iso=0.0, stream=side.cuda_stream, **MARCH_SETS[names[0]])
    side.synchronize()
    assert hits.intact() and hits.bytes().tobytes() == refs[0].tobytes()


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
        dims = (17, 9, 5)
        val, o, sp = _field("sphere", dims)
        rays, p = _march_rays(65, False, False), _mixed_points(dims, o, sp, 65)
        a.sample_grid(val, o, sp, p)
        a.march_grid(val, o, sp, rays)
        a.debug_march_work(val, o, sp, rays)
        tv = torch.from_numpy(val.copy()).cuda()
        a.sample_grid_tensor(tv, o, sp, torch.from_numpy(p.copy()).cuda())
        a.march_grid_tensor(tv, o, sp, torch.from_numpy(rays.copy()).cuda())
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


def test_end_to_end_offset_surface_of_the_cube(pkg, sc, scene_data):
    """The cube's signed distances on 33^3, marched at iso = 0.25 of the extent.  Every HIT point p has |sdf(p) - iso| <= h sqrt(3) +
    hit_eps (a trilinear value lies between its corners' values, and those differ from a 1-Lipschitz field at p by at most the cell's
    diagonal; the bisection brings the trilinear value itself to the level); rays that miss the cube's box dilated by iso + h sqrt(3)
    are MISS."""
    pos = np.asarray(scene_data("cube").pos_nrm, F).reshape(-1, 6)[:, :3].astype(np.float64)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    extent = float((hi - lo).max())
    iso, hit_eps, n = 0.25 * extent, 1e-4 * extent, 33
    origin = (lo - 0.6 * extent).astype(F)
    spacing = ((hi - lo + 1.2 * extent) / (n - 1)).astype(F)
    h = float(spacing.max())
    values = sc.sdf_grid_tensor(origin, spacing, (n, n, n), want="sdf")
    W = H = 64
    rays = sc.generate_rays(pkg.scenes.default_camera(W, H), W, H)
    flat = np.ascontiguousarray(rays).view(F).reshape(-1, 7).copy()
    flat[:, 6] = np.finfo(F).max
    prm = dict(iso=iso, relax=1.0, min_step=1e-4 * extent, hit_eps=hit_eps, max_steps=512, refine=16)
    res = sc.march_grid_tensor(values, origin, spacing, torch.from_numpy(flat).cuda(), **prm)
    rec = res["records"].cpu().numpy().view(gref.HIT_DTYPE).reshape(-1)
    want, _ = gref.march(values.cpu().numpy(), origin, spacing, flat, **prm)
    assert rec.tobytes() == want.tobytes()
    hit = rec["status"] == gref.HIT
    assert 200 < hit.sum() < len(rec) and not np.isin(rec["status"], (gref.EXHAUSTED, gref.NONFINITE)).any()
    p = (flat[hit, 0:3] + rec["t"][hit, None] * flat[hit, 3:6]).astype(F)
    sdf = sc.sdf(p, want="sdf").astype(np.float64)
    off = np.abs(sdf - iso)
    print("largest |sdf(p) - iso|:", off.max(), "bound:", h * 3 ** 0.5 + hit_eps)
    assert off.max() <= h * 3 ** 0.5 + hit_eps
    # the cube's box, dilated, as a scene of twelve triangles
    r = iso + h * 3 ** 0.5
    blo, bhi = lo - r, hi + r
    corners = np.asarray([[(blo, bhi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)], F)
    tris = np.asarray([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5],
                       [3, 7, 5]], np.uint32)
    box = pkg.Scene(pkg.scenes.mesh_scene_data(corners, tris), device=0)
    try:
        misses_box = ~box.occluded(flat)
    finally:
        box.close()
    assert np.all(rec["status"][misses_box] == gref.MISS)

"""GPU: surface sampling (cgrt_sample_surface*; include/cgrt.h "Surface sampling").  Byte comparisons against the numpy
restatement (tests/sampling_ref.py), whose statistics tests/test_sampling_cpu.py holds.

* Records, host form and device form, on cube, cornell, monkey, dodge and the 8-triangle degenerate scene; n in {1, 63, 64, 65, 4097};
  seeds {0, 1, 2^63 + 5}; independent, strata == n, and strata == 3 n with first == n; first = 2^32 - 3 with n = 8 (the counter's high
  word); 65 536 samples of the 800 000-triangle dragon stand-in (twenty search levels, repeated thresholds).
* Chunking: two calls of 1 000 on two streams equal one call of 2 000, in both modes.
* Empty scenes: miss records, zero rows.
* Table rows for C in {1, 3, 4, 7, 256}, pointers aligned and offset by 4 bytes (the 16-byte and the scalar path of rows and records);
  with the vertex positions as the table the rows are the records' points.
* closest_points of the sampled points on monkey: dist2 <= 3 (4 * 2^-24 * S)^2.
* The tensor form's views and out= reuse; a device-form call on a side stream does not wait for the default stream; four host threads
  get the single-thread bytes; a device span that is too small is CGRT_E_ARG with nothing written; the prediction record, the hint
  state and the layout do not move."""
import ctypes as C
import dataclasses
import threading
import time

import numpy as np
import pytest

import sampling_ref as sref
from conftest import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
SCENES = ("cube", "cornell", "monkey", "dodge", "degenerate8")
LENGTHS = (1, 63, 64, 65, 4097)
SEEDS = (0, 1, (1 << 63) + 5)
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")

_scenes = {}


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    """name -> (SceneData, Scene on device 0, the restatement's table), created once."""

    def get(name):
        if name not in _scenes:
            sd = {"degenerate8": lambda: sref.degenerate_scene(pkg), "dragon800k": lambda: pkg.scenes.make_dragon(800_000),
                  "spheres": pkg.scenes.spheres_preset}.get(name, lambda: scene_data(name))()
            _scenes[name] = (sd, pkg.Scene(sd, device=0), sref.table(sd))
        return _scenes[name]

    yield get
    for _, sc, _ in _scenes.values():
        sc.close()
    _scenes.clear()


class Guarded:
    """nbytes of device memory between two guards, all of it sentinel bytes before the call; `shift` moves it off 16-byte alignment."""

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


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _records(raw):
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view(sref.SAMPLE_DTYPE)


def _same_records(got, want, what):
    got, want = _records(got), _records(want)
    assert len(got) == len(want), what
    bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 8) != want.view(np.uint32).reshape(-1, 8)).any(1))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def _modes(n):
    return (dict(first=0, strata=0), dict(first=0, strata=n), dict(first=n, strata=3 * n))


def _device_records(sc, n, shift=0, **kw):
    g = Guarded(32 * n, shift)
    sc.sample_surface_device(n, g.ptr(), stream=torch.cuda.current_stream().cuda_stream, **kw)
    assert g.intact(), ("guards", n, kw)
    return g.bytes()


# ---- 1. records ----
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", SCENES)
def test_records_equal_the_restatement(pkg, scenes, name, form):
    sd, sc, tab = scenes(name)
    for n in LENGTHS:
        for seed in SEEDS:
            for mode in _modes(n):
                want, _ = sref.sample(sd, n, seed=seed, tab=tab, **mode)
                got = sc.sample_surface(n, seed=seed, **mode) if form == "host" else _device_records(sc, n, seed=seed, **mode)
                _same_records(got, want, (name, form, n, seed, mode))
    assert (want["prim_id"] < sd.ntris).all() and np.array_equal(want["mesh_id"], np.asarray(sd.tri_mesh)[want["prim_id"]])


@pytest.mark.parametrize("form", ["host", "device"])
def test_the_counters_high_word(pkg, scenes, form):
    sd, sc, tab = scenes("monkey")
    first = (1 << 32) - 3
    want, _ = sref.sample(sd, 8, seed=7, first=first, tab=tab)
    got = sc.sample_surface(8, seed=7, first=first) if form == "host" else _device_records(sc, 8, seed=7, first=first)
    _same_records(got, want, form)
    low, _ = sref.sample(sd, 5, seed=7, first=0, tab=tab)
    assert not np.array_equal(want["bary"][3:], low["bary"]), "sample 2^32 + k is not sample k"


def test_the_large_scene(pkg, scenes):
    sd, sc, tab = scenes("dragon800k")
    _, _, T, last = tab
    assert last >= 1 << 19, "twenty search levels"
    n = 65536
    for mode in (dict(strata=0), dict(strata=n)):
        want, _ = sref.sample(sd, n, seed=3, tab=tab, **mode)
        _same_records(_device_records(sc, n, seed=3, **mode), want, mode)
    _same_records(sc.sample_surface(4097, seed=3), sref.sample(sd, 4097, seed=3, tab=tab)[0], "host form")


# ---- 2. chunking ----
@pytest.mark.parametrize("strata", [0, 2000])
def test_chunks_on_two_streams_equal_one_call(pkg, scenes, strata):
    sd, sc, tab = scenes("dodge")
    whole = _device_records(sc, 2000, seed=11, strata=strata)
    _same_records(whole, sref.sample(sd, 2000, seed=11, strata=strata, tab=tab)[0], "one call")
    g = Guarded(32 * 2000)
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    sc.sample_surface_device(1000, g.ptr() + 32 * 1000, seed=11, first=1000, strata=strata, stream=s1.cuda_stream)
    sc.sample_surface_device(1000, g.ptr(), seed=11, first=0, strata=strata, stream=s0.cuda_stream)
    s0.synchronize()
    s1.synchronize()
    assert g.intact() and g.bytes().tobytes() == whole.tobytes()
    host = np.concatenate([sc.sample_surface(k, seed=11, first=f, strata=strata) for f, k in ((0, 1), (1, 999), (1000, 1000))])
    assert host.tobytes() == whole.tobytes()


# ---- 3. empty scenes ----
@pytest.mark.parametrize("name", ["flat", "spheres"])
def test_empty_scenes_give_miss_records_and_zero_rows(pkg, scenes, name):
    if name == "flat":
        sd = sref.degenerate_scene(pkg)
        sd = dataclasses.replace(sd, tri=np.asarray(sd.tri).reshape(-1, 3)[[0, 3, 4, 7]].copy(), tri_mesh=np.zeros(4, np.uint32), name="flat")
        sc = pkg.Scene(sd, device=0)
    else:
        sd, sc, _ = scenes("spheres")
    try:
        nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
        miss = np.zeros(70, sref.SAMPLE_DTYPE)
        miss["mesh_id"], miss["prim_id"] = 0xFFFFFFFF, pkg.NO_PRIM
        for kw in (dict(), dict(strata=100, first=30)):
            _same_records(sc.sample_surface(70, seed=4, **kw), miss, (name, kw))
            _same_records(_device_records(sc, 70, seed=4, **kw), miss, (name, kw))
        if nverts:
            rec, rows = sc.sample_surface(70, attr=np.ones((nverts, 5), np.float32))
            _same_records(rec, miss, name)
            assert rows.shape == (70, 5) and not rows.view(np.uint32).any()
            rows_g = Guarded(70 * 5 * 4)
            attr = torch.ones((nverts, 5), dtype=torch.float32, device="cuda")
            rec_g = Guarded(70 * 32)
            sc.sample_surface_device(70, rec_g.ptr(), d_attr_ptr=attr.data_ptr(), channels=5, d_out_attr_ptr=rows_g.ptr())
            assert rows_g.intact() and rec_g.intact() and not rows_g.bytes().any() and rec_g.bytes().tobytes() == miss.tobytes()
        assert sc.debug_sample_table()["last"] == pkg.NO_PRIM
    finally:
        if name == "flat":
            sc.close()


# ---- 4. table rows ----
@pytest.mark.parametrize("shift", [0, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("channels", [1, 3, 4, 7, 256])
def test_table_rows_equal_the_restatement(pkg, scenes, channels, shift):
    sd, sc, tab = scenes("monkey")
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    attr = np.random.default_rng(channels).standard_normal((nverts, channels)).astype(np.float32)
    g_attr = Guarded(attr.nbytes, shift)
    g_attr.buf[g_attr.lo : g_attr.lo + attr.nbytes] = torch.from_numpy(attr.view(np.uint8).reshape(-1)).cuda()
    for n, kw in ((1, dict()), (65, dict(strata=65)), (1000, dict(first=5))):
        want, want_rows = sref.sample(sd, n, seed=9, attr=attr, tab=tab, **kw)
        rec, rows = sc.sample_surface(n, seed=9, attr=attr, **kw)
        _same_records(rec, want, ("host", n))
        assert rows.shape == want_rows.shape and same_bits(rows, want_rows).all(), ("host rows", n)
        g_rec, g_rows = Guarded(32 * n, shift), Guarded(4 * n * channels, shift)
        sc.sample_surface_device(n, g_rec.ptr(), seed=9, d_attr_ptr=g_attr.ptr(), channels=channels, d_out_attr_ptr=g_rows.ptr(), **kw)
        assert g_rec.intact() and g_rows.intact() and g_attr.intact()
        _same_records(g_rec.bytes(), want, ("device", n, shift))
        assert g_rows.bytes().tobytes() == want_rows.tobytes(), ("device rows", n, shift)


def test_positions_as_the_table_give_the_points(pkg, scenes):
    sd, sc, _ = scenes("dodge")
    pos = np.ascontiguousarray(np.asarray(sd.pos_nrm, np.float32).reshape(-1, 6)[:, 0:3])
    rec, rows = sc.sample_surface(5000, seed=2, attr=pos)
    assert np.array_equal(rows.view(np.uint32), rec["point"].view(np.uint32))
    t = sc.sample_surface_tensor(5000, seed=2, attr=torch.from_numpy(pos).cuda())
    assert np.array_equal(_np(t["attr"]).view(np.uint32), rec["point"].view(np.uint32))
    assert np.array_equal(_np(t["point"]).view(np.uint32), rec["point"].view(np.uint32))


# ---- 5. the family ----
def test_closest_points_finds_the_samples_on_the_surface(pkg, scenes):
    sd, sc, _ = scenes("monkey")
    rec = sc.sample_surface(20000, seed=6)
    S = np.abs(np.concatenate(sref.vertices(sd), 1)).max(1)[rec["prim_id"]].astype(np.float64)
    d2 = sc.closest_points(rec["point"])["dist2"].astype(np.float64)
    print("largest dist2 / (3 (4 2^-24 S)^2):", float((d2 / (3 * (4 * 2.0 ** -24 * S) ** 2)).max()))
    assert (d2 <= 3 * (4 * 2.0 ** -24 * S) ** 2).all()


# ---- 6. forms ----
def test_tensor_form_returns_views_and_reuses_out(pkg, scenes):
    sd, sc, tab = scenes("cornell")
    n = 300
    want, _ = sref.sample(sd, n, seed=5, strata=n, tab=tab)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    r = sc.sample_surface_tensor(n, seed=5, strata=n, stream=side)
    side.synchronize()
    assert set(r) == {"point", "mesh_id", "prim_id", "bary", "out"}
    o = r["out"]
    assert tuple(o.shape) == (n, 8) and o.dtype == torch.float32 and o.device.index == 0
    assert r["prim_id"].dtype == torch.int32 and r["mesh_id"].dtype == torch.int32
    for k, sl in (("point", slice(0, 3)), ("bary", slice(5, 8))):
        assert r[k].data_ptr() == o[:, sl].data_ptr() and tuple(r[k].shape) == (n, 3), k
    assert r["mesh_id"].data_ptr() == o.data_ptr() + 12 and r["prim_id"].data_ptr() == o.data_ptr() + 16
    _same_records(_np(o), want, "tensor form")
    assert np.array_equal(_np(r["prim_id"]).view(np.uint32), want["prim_id"])
    again = sc.sample_surface_tensor(n, seed=6, out=o)
    assert again["out"] is o
    _same_records(_np(o), sref.sample(sd, n, seed=6, tab=tab)[0], "out= reused")
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    attr = torch.rand((nverts, 4), device="cuda")
    rows = torch.empty((n, 4), device="cuda")
    r = sc.sample_surface_tensor(n, seed=6, attr=attr, out=o, out_attr=rows)
    assert r["attr"] is rows and r["out"] is o
    assert same_bits(_np(rows), sref.sample(sd, n, seed=6, attr=_np(attr), tab=tab)[1]).all()
    empty = sc.sample_surface_tensor(0)
    assert tuple(empty["out"].shape) == (0, 8)
    for bad in (dict(out=torch.empty((n + 1, 8), device="cuda")), dict(out=torch.empty((n, 8))), dict(out_attr=rows),
                dict(attr=attr[:, :3]), dict(attr=attr, out_attr=torch.empty((n, 3), device="cuda"))):
        with pytest.raises(ValueError):
            sc.sample_surface_tensor(n, **bad)


def _sleep_cycles(seconds):
    return int(seconds * 1e9 * 2.4)  # (~2.4 GHz shader clock; only the order of magnitude matters)


def test_device_form_on_a_side_stream_does_not_wait_for_the_default_stream(pkg, scenes):
    sd, sc, tab = scenes("monkey")
    n = 4097
    side = torch.cuda.Stream()
    out = torch.empty((n, 8), device="cuda")
    sc.sample_surface_tensor(n, seed=1, out=out, stream=side)  # (warm: the tables are on the device)
    torch.cuda.synchronize()
    out.zero_()
    torch.cuda.synchronize()
    torch.cuda._sleep(_sleep_cycles(0.2))  # on the default stream
    busy = torch.cuda.Event()
    busy.record()
    t0 = time.perf_counter()
    sc.sample_surface_device(n, out.data_ptr(), seed=2, stream=side.cuda_stream)
    dt = time.perf_counter() - t0
    side.synchronize()
    pending = not busy.query()
    torch.cuda.synchronize()
    assert dt < 0.05, f"the call took {dt * 1e3:.1f} ms"
    assert pending, "the side stream's samples were held back by the default stream"
    _same_records(_np(out), sref.sample(sd, n, seed=2, tab=tab)[0], "side stream")


def test_four_threads_get_the_single_thread_bytes(pkg, scene_data):
    sd = scene_data("dodge")
    sc = pkg.Scene(sd, device=0)  # (fresh: the threads race to build the tables)
    try:
        nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
        base = sc.device_bytes()
        attr = np.random.default_rng(1).standard_normal((nverts, 3)).astype(np.float32)
        jobs = [dict(n=1500 + 7 * k, seed=k, first=100 * k, strata=0 if k % 2 else 5000) for k in range(8)]
        got, errors = {}, []

        def work(tid):
            try:
                for it in range(3):
                    for k in range(tid, len(jobs), 4):
                        got[(tid, it, k)] = sc.sample_surface(attr=attr if (k + it) % 2 else None, **jobs[k])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert len(got) == 3 * len(jobs)
        tab = sref.table(sd)
        for (tid, it, k), res in got.items():
            want, rows = sref.sample(sd, attr=attr, tab=tab, **jobs[k])
            if (k + it) % 2:
                _same_records(res[0], want, (tid, it, k))
                assert same_bits(res[1], rows).all(), (tid, it, k)
            else:
                _same_records(res, want, (tid, it, k))
        assert sc.device_bytes() == base + 20 * sd.ntris, "each table was uploaded once"
    finally:
        sc.close()


def test_device_form_checks_its_spans(pkg, scenes):
    sd, sc, _ = scenes("cube")
    n = 1 << 18
    hip = C.CDLL(pkg.LIB_PATH)
    out = torch.full((n, 8), 7.0, device="cuda")
    rows = torch.full((n, 4), 7.0, device="cuda")
    attr = torch.ones((8, 4), device="cuda")
    host = np.zeros(64, np.float32)
    torch.cuda.synchronize()
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), C.c_size_t(4096)) == 0
    try:
        assert hip.hipMemset(small, 0x5A, C.c_size_t(4096)) == 0
        cases = [dict(d_out_ptr=small.value), dict(d_out_ptr=host.ctypes.data),
                 dict(d_out_ptr=out.data_ptr(), d_attr_ptr=attr.data_ptr(), channels=4, d_out_attr_ptr=small.value),
                 dict(d_out_ptr=out.data_ptr(), d_attr_ptr=small.value, channels=256, d_out_attr_ptr=rows.data_ptr()),
                 dict(d_out_ptr=out.data_ptr(), d_attr_ptr=host.ctypes.data, channels=4, d_out_attr_ptr=rows.data_ptr())]
        for kw in cases:
            with pytest.raises(pkg.CgrtError) as e:
                sc.sample_surface_device(n if kw.get("channels") != 256 else 1000, **kw)
            assert e.value.code == -1, kw
        torch.cuda.synchronize()
        back = np.zeros(4096, np.uint8)
        assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), small, C.c_size_t(4096), 2) == 0
        assert (back == 0x5A).all() and (_np(out) == 7.0).all() and (_np(rows) == 7.0).all(), "refused before any work"
    finally:
        assert hip.hipFree(small) == 0
    sc.sample_surface_device(0, 0)  # n == 0 touches nothing


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
        base = a.device_bytes()
        a.sample_surface_device(0, 0)
        a.sample_surface(0)
        a.triangle_areas()
        a.debug_sample_table()
        assert a.device_bytes() == base, "n == 0 and the host entries upload nothing"
        first = a.sample_surface(1000, seed=1)
        assert a.device_bytes() == base + 20 * sd.ntris, "the thresholds (4 bytes per triangle) and the lookup table (16)"
        nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
        a.sample_surface(1000, seed=1, strata=1000, attr=np.ones((nverts, 3), np.float32))
        a.sample_surface_tensor(5000, seed=2, attr=torch.ones((nverts, 8), device="cuda"))
        torch.cuda.synchronize()
        assert a.sample_surface(1000, seed=1).tobytes() == first.tobytes()
        assert a.device_bytes() == base + 20 * sd.ntris, "once"
        ref = b.render(cam, W, H)
        for _ in range(2):
            ref = b.render(cam, W, H)
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes() + 20 * sd.ntris
    finally:
        a.close()
        b.close()

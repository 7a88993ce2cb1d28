"""GPU: Poisson-disk sets (cgrt_poisson_disk*; include/cgrt.h "Poisson-disk sets").  Byte comparisons against the numpy
restatement (tests/poisson_ref.py), whose own properties tests/test_poisson_cpu.py holds.

* Candidates from sample_surface on cube, monkey and dodge; n in {1, 2, 63, 64, 65, 4097}; seeds {0, 1, 2^63 + 5} (of the samples and of
  the order); min_dist2 = k A / (pi n) for k in {1, 10, 100} -- a disk of that radius on a surface of area A holds k of n samples --; the
  host, device and brute forms.
* The two fixed cases of the CPU tests; the line's device run takes 2 .. 512 rounds (it may decide earlier than the synchronous form,
  never differently) and goes through many read-back batches.
* n copies of one point; all priorities equal; NaN and inf coordinates; min_dist2 in {0, -1, NaN}; min_dist2 = 3e38 on a unit cloud.
* Scale: min_dist2 times 2^+-40 and 2^+-80 with the points times 2^+-20 and 2^+-40 (d2 scales by the square of the points' factor, and
  a factor of 2^+-80 on the points would take d2 out of f32's range) gives the unscaled flags; clusters spread over [-2^20, 2^20] with
  radius 1 (large cell coordinates, coordinates 1/8 apart).
* The grid form against the brute form on 65 536 candidates of the 800 000-triangle dragon stand-in, at about 8 and about 64 conflicts.
* sample_surface_poisson_tensor equals the composition by hand.
* Guard bytes around keep and the workspace (which sits 8 bytes off a 16-byte boundary and is filled with 0xA5, or zeros) are intact; a
  workspace one byte short is CGRT_E_ARG with nothing written; four host threads get the single-thread bytes; a call on a side stream
  gives the same bytes; the prediction record, the hint state and the layout do not move."""
import math
import threading

import numpy as np
import pytest

import poisson_ref as pref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
SCENES = ("cube", "monkey", "dodge")
LENGTHS = (1, 2, 63, 64, 65, 4097)
SEEDS = (0, 1, (1 << 63) + 5)
CONFLICTS = (1, 10, 100)
KEYS = ("primary_rays", "shadow_rays", "reflection_rays", "soft_shadow_rays", "levels")

_scenes = {}
_refs = {}


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    """name -> (SceneData, Scene on device 0, total area), created once."""

    def get(name):
        if name not in _scenes:
            sd = pkg.scenes.make_dragon(800_000) if name == "dragon800k" else scene_data(name)
            sc = pkg.Scene(sd, device=0)
            _scenes[name] = (sd, sc, sc.triangle_areas()[1])
        return _scenes[name]

    yield get
    for _, sc, _ in _scenes.values():
        sc.close()
    _scenes.clear()
    _refs.clear()


def _m(area, n, k):
    return np.float32(k * area / (math.pi * n))


def _reference(scenes, name, n, seed):
    """(points, {k: (min_dist2, flags)}) of n candidates: computed once, shared by the forms, never changed."""
    key = (name, n, seed)
    if key not in _refs:
        _, sc, area = scenes(name)
        p = np.ascontiguousarray(sc.sample_surface(n, seed=seed)["point"])
        d2 = pref.d2_matrix(p)
        res = {}
        for k in CONFLICTS:
            keep = pref.greedy(p, _m(area, n, k), seed=seed, d2=d2)
            keep.setflags(write=False)
            res[k] = (_m(area, n, k), keep)
        p.setflags(write=False)
        _refs[key] = (p, res)
    return _refs[key]


class Guarded:
    """nbytes of device memory between two guards, all of it `fill` bytes before the call; `shift` moves it off 16-byte alignment."""

    def __init__(self, nbytes, shift=0, fill=SENTINEL):
        self.n, self.lo = int(nbytes), PAD + shift
        self.buf = torch.full((self.n + 2 * PAD + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        if fill != SENTINEL:
            self.buf[self.lo : self.lo + self.n] = fill

    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def bytes(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[self.lo : self.lo + self.n]

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[: self.lo] == SENTINEL).all() and (b[self.lo + self.n :] == SENTINEL).all())


def _device(sc, p, m, seed=0, priority=None, fill=SENTINEL, stream=None):
    """The device form with guards around keep and the workspace: (n,) bool."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    n = len(p)
    pts = torch.from_numpy(p.copy()).cuda()
    pr = None if priority is None else torch.from_numpy(np.asarray(priority, np.uint32).view(np.int32).copy()).cuda()
    nbytes = sc.poisson_disk_workspace(n)
    keep, ws = Guarded(n), Guarded(nbytes, shift=8, fill=fill)
    torch.cuda.synchronize()
    kept = sc.poisson_disk_device(pts.data_ptr(), n, float(m), keep.ptr(), ws.ptr(), nbytes, seed=seed,
                                  d_priority_ptr=0 if pr is None else pr.data_ptr(),
                                  stream=(stream or torch.cuda.current_stream()).cuda_stream)
    assert keep.intact() and ws.intact(), ("guards", n, float(m))
    b = keep.bytes()
    assert set(np.unique(b)) <= {0, 1} and int(b.sum()) == kept
    return b.astype(bool)


def _form(sc, form, p, m, seed=0, priority=None):
    if form == "host":
        return sc.poisson_disk(p, float(m), seed=seed, priority=priority)
    if form == "brute":
        return sc.poisson_disk_brute(p, float(m), seed=seed, priority=priority)
    return _device(sc, p, m, seed=seed, priority=priority)


def _same(got, want, what):
    got, want = np.asarray(got, bool), np.asarray(want, bool)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, len(bad), int(bad[0]), int(got.sum()), int(want.sum()))


FORMS = ("host", "device", "brute")


# ---- 1. candidates on the fixtures ----
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", SCENES)
def test_flags_equal_the_restatement(pkg, scenes, name, form):
    _, sc, _ = scenes(name)
    for n in LENGTHS:
        for seed in SEEDS:
            p, res = _reference(scenes, name, n, seed)
            for k in CONFLICTS:
                m, want = res[k]
                _same(_form(sc, form, p, m, seed=seed), want, (name, form, n, seed, k))
    counts = [int(res[k][1].sum()) for k in CONFLICTS]
    assert counts[0] > counts[1] > counts[2] >= 1, ("a larger radius keeps fewer of the 4097", counts)


def test_mean_conflicts_are_what_the_radii_aim_for(scenes):
    """the radii of test 1 on its largest set: about 1, 10 and 100 conflicts per candidate (within a factor of 2.5: edges, curvature)"""
    for name in SCENES:
        _, _, area = scenes(name)
        p, _ = _reference(scenes, name, 4097, 0)
        d2 = pref.d2_matrix(p)
        for k in CONFLICTS:
            mean = pref.conflicts(p, _m(area, 4097, k), d2).sum() / 4097
            assert k / 2.5 <= mean <= k * 2.5, (name, k, mean)


# ---- 2. the fixed cases ----
@pytest.mark.parametrize("form", FORMS)
def test_line_case(scenes, form):
    _, sc, _ = scenes("cube")
    p, m, prio = pref.line_case()
    got = _form(sc, form, p, m, priority=prio)
    assert np.array_equal(np.flatnonzero(got), np.arange(0, 512, 2))
    if form == "host":
        w = sc.debug_poisson_work(p, float(m), priority=prio)
        assert 2 <= w["rounds"] <= 512, w
        assert w["pair_tests"] >= 511 and 1 <= w["buckets_used"] <= w["buckets"], w


@pytest.mark.parametrize("form", FORMS)
def test_lattice_case(scenes, form):
    _, sc, _ = scenes("cube")
    p = pref.lattice_case()
    assert _form(sc, form, p, 0.0625).all(), "a neighbour at exactly the radius does not conflict"
    up = np.nextafter(np.float32(0.0625), np.float32(1))
    for seed in SEEDS:
        _same(_form(sc, form, p, up, seed=seed), pref.greedy(p, up, seed=seed), (form, seed))


# ---- 3. degenerate inputs ----
@pytest.mark.parametrize("form", FORMS)
def test_copies_of_one_point_and_equal_priorities(scenes, form):
    _, sc, _ = scenes("cube")
    n = 300
    p = np.tile(np.asarray([[0.25, -3.0, 7.5]], np.float32), (n, 1))
    for seed in SEEDS:
        first = int(np.argmin(pref.keys(n, seed)))
        got = _form(sc, form, p, 1.0, seed=seed)
        assert np.array_equal(np.flatnonzero(got), [first]), (seed, first)
    assert np.array_equal(np.flatnonzero(_form(sc, form, p, 1.0, priority=np.full(n, 9, np.uint32))), [0])
    rng = np.random.default_rng(11)
    q = rng.random((1000, 3)).astype(np.float32)
    want = pref.greedy(q, 0.01, priority=np.arange(1000))
    for c in (0, 0xFFFFFFFF):
        _same(_form(sc, form, q, 0.01, priority=np.full(1000, c, np.uint32)), want, ("equal priorities: the order is the index", c))


def _bad_cloud(n=1500, seed=5):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)).astype(np.float32)
    idx = rng.choice(n, n // 10, replace=False)
    p[idx, rng.integers(0, 3, len(idx))] = rng.choice(np.asarray([np.nan, np.inf, -np.inf], np.float32), len(idx))
    p[idx[:5]] = np.nan
    return p


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_points_and_radii_without_conflicts(scenes, form):
    _, sc, _ = scenes("cube")
    p = _bad_cloud()
    fin = pref.finite(p)
    assert 0 < (~fin).sum() < len(p)
    d2 = pref.d2_matrix(p)
    for m in (0.002, 0.02):
        want = pref.greedy(p, m, seed=3, d2=d2)
        assert not (want & ~fin).any()
        _same(_form(sc, form, p, m, seed=3), want, (form, m))
    for m in (0.0, -1.0, float("nan"), -float("inf")):
        _same(_form(sc, form, p, m), fin, (form, m))
    allbad = np.full((70, 3), np.nan, np.float32)
    assert not _form(sc, form, allbad, 1.0).any()


@pytest.mark.parametrize("form", FORMS)
def test_a_radius_that_covers_the_cloud_keeps_one_point(scenes, form):
    _, sc, _ = scenes("cube")
    p = _bad_cloud(2000, 8)
    fin = np.flatnonzero(pref.finite(p))
    for seed in SEEDS:
        k = pref.keys(len(p), seed)
        first = int(fin[np.argmin(k[fin])])
        assert np.array_equal(np.flatnonzero(_form(sc, form, p, 3e38, seed=seed)), [first]), (form, seed)


# ---- 4. scale ----
@pytest.mark.parametrize("form", ("host", "device"))
def test_scaled_points_and_radius_give_the_same_flags(scenes, form):
    p, res = _reference(scenes, "monkey", 4097, 1)
    _, sc, _ = scenes("monkey")
    for k in (10, 100):
        m, want = res[k]
        for e in (-40, -20, 20, 40):
            ps, ms = p * np.float32(2.0 ** e), np.float32(m * np.float32(2.0 ** (2 * e)))
            assert np.isfinite(ms) and ms > 0 and np.isfinite(ps).all()
            _same(_form(sc, form, ps, ms, seed=1), want, (form, k, e))


@pytest.mark.parametrize("form", FORMS)
def test_large_coordinates(scenes, form):
    """256 clusters of 16 points, centres spread over [-2^20, 2^20]^3, offsets multiples of 1/8 (the spacing of f32 there) within +-1.5"""
    _, sc, _ = scenes("cube")
    rng = np.random.default_rng(21)
    centres = np.round(rng.uniform(-(2.0 ** 20), 2.0 ** 20, (256, 1, 3)))
    p = (centres + rng.integers(-12, 13, (256, 16, 3)) / 8.0).reshape(-1, 3).astype(np.float32)
    p[0], p[1] = -(2.0 ** 20), 2.0 ** 20
    want = pref.greedy(p, 1.0, seed=2)
    assert 256 < want.sum() < len(p)
    _same(_form(sc, form, p, 1.0, seed=2), want, form)


# ---- 5. the grid against the brute form at size ----
def test_grid_equals_brute_on_the_dragon(scenes):
    _, sc, area = scenes("dragon800k")
    n = 65536
    p = np.ascontiguousarray(sc.sample_surface(n, seed=4, strata=n)["point"])
    for k in (8, 64):
        m = _m(area, n, k)
        grid, brute = sc.poisson_disk(p, float(m), seed=4), sc.poisson_disk_brute(p, float(m), seed=4)
        _same(grid, brute, ("dragon", k))
        assert n / (4 * k) <= grid.sum() <= n, (k, int(grid.sum()))
        sub = np.flatnonzero(grid)[:4096]
        assert not pref.conflicts(p[sub], m).any(), "kept points do not conflict (the first 4 096 of them, all pairs)"
        _same(_device(sc, p, m, seed=4), grid, ("dragon, device form", k))


# ---- 6. the composition ----
def test_sample_surface_poisson_tensor_is_the_composition(scenes):
    sd, sc, area = scenes("monkey")
    n, seed = 5000, 7
    nverts = len(np.asarray(sd.pos_nrm).reshape(-1, 6))
    attr = torch.from_numpy(np.random.default_rng(2).standard_normal((nverts, 3)).astype(np.float32)).cuda()
    for strata in (True, False):
        m = float(_m(area, n, 10))
        got = sc.sample_surface_poisson_tensor(n, m, seed=seed, strata=strata, attr=attr)
        cand = sc.sample_surface_tensor(n, seed=seed, strata=n if strata else 0, attr=attr)
        mask = sc.poisson_disk_tensor(cand["point"].contiguous(), m, seed=seed)
        torch.cuda.synchronize()
        host = sc.poisson_disk(cand["point"].cpu().numpy(), m, seed=seed)
        assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), host)
        idx = np.flatnonzero(host)
        assert np.array_equal(got["index"].cpu().numpy(), idx) and 0 < len(idx) < n
        assert set(got) == set(cand) | {"index"}
        for key in cand:
            assert np.array_equal(got[key].cpu().numpy().view(np.uint8), cand[key][torch.from_numpy(idx).cuda()].cpu().numpy().view(np.uint8)), key
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(sc.poisson_disk_workspace(n) + 8, dtype=torch.uint8, device="cuda")
    assert sc.poisson_disk_tensor(cand["point"].contiguous(), m, seed=seed, out=out, workspace=ws) is out
    assert np.array_equal(out.cpu().numpy().astype(bool), host)


# ---- 7. guards, the workspace, threads, streams ----
def test_workspace_contents_do_not_matter_and_a_short_one_is_refused(pkg, scenes):
    _, sc, area = scenes("dodge")
    p, res = _reference(scenes, "dodge", 4097, 0)
    m, want = res[10]
    for fill in (SENTINEL, 0x00, 0xFF):
        _same(_device(sc, p, m, fill=fill), want, fill)
    n = len(p)
    pts = torch.from_numpy(p.copy()).cuda()
    nbytes = sc.poisson_disk_workspace(n)
    keep, ws = Guarded(n), Guarded(nbytes)
    for kw in (dict(d_workspace_ptr=ws.ptr(), workspace_bytes=nbytes - 1), dict(d_workspace_ptr=ws.ptr() + 4, workspace_bytes=nbytes),
               dict(d_workspace_ptr=0, workspace_bytes=nbytes)):
        with pytest.raises(pkg.CgrtError) as e:
            sc.poisson_disk_device(pts.data_ptr(), n, float(m), keep.ptr(), **kw)
        assert e.value.code == -1, kw
    # a workspace that is large enough by its argument but not as device memory: refused by the span check, before any work
    host = np.zeros(nbytes + 16, np.uint8)
    with pytest.raises(pkg.CgrtError) as e:
        sc.poisson_disk_device(pts.data_ptr(), n, float(m), keep.ptr(), host.ctypes.data + (-host.ctypes.data) % 8, nbytes)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert (keep.bytes() == SENTINEL).all() and (ws.bytes() == SENTINEL).all() and keep.intact() and ws.intact(), "refused before any work"
    assert not host.any()
    assert sc.poisson_disk_device(0, 0, 1.0, 0, 0, 0) == 0, "n == 0 touches nothing"
    assert sc.poisson_disk(np.zeros((0, 3), np.float32), 1.0).shape == (0,)


def test_four_threads_get_the_single_thread_bytes(pkg, scenes):
    _, sc, _ = scenes("monkey")
    jobs = []
    for k, (n, seed) in enumerate(((4097, 0), (4097, 1), (65, 0), (4097, (1 << 63) + 5), (63, 1), (64, 0), (2, 1), (4097, 1))):
        p, res = _reference(scenes, "monkey", n, seed)
        m, want = res[CONFLICTS[k % 3]]
        jobs.append((p, float(m), seed, want))
    got, errors = {}, []

    def work(tid):
        try:
            for it in range(3):
                for k in range(tid, len(jobs), 4):
                    p, m, seed, _ = jobs[k]
                    got[(tid, it, k)] = (sc.poisson_disk_brute if (k + it) % 3 == 0 else sc.poisson_disk)(p, m, seed=seed)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got) == 3 * len(jobs)
    for (tid, it, k), res in got.items():
        _same(res, jobs[k][3], (tid, it, k))


def test_a_side_stream_gives_the_same_bytes(scenes):
    _, sc, _ = scenes("dodge")
    p, res = _reference(scenes, "dodge", 4097, 1)
    side = torch.cuda.Stream()
    for k in CONFLICTS:
        m, want = res[k]
        _same(_device(sc, p, m, seed=1, stream=side), want, ("side stream", k))
        pts = torch.from_numpy(p.copy()).cuda()
        torch.cuda.synchronize()
        _same(sc.poisson_disk_tensor(pts, float(m), seed=1, stream=side).cpu().numpy(), want, ("tensor form, side stream", k))


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
        p = np.random.default_rng(3).random((3000, 3)).astype(np.float32)
        first = a.poisson_disk(p, 0.004, seed=1)
        a.poisson_disk_brute(p, 0.004, seed=1)
        a.debug_poisson_work(p, 0.004, seed=1)
        a.poisson_disk_tensor(torch.from_numpy(p).cuda(), 0.004, seed=2)
        torch.cuda.synchronize()
        assert a.poisson_disk(p, 0.004, seed=1).tobytes() == first.tobytes()
        assert a.device_bytes() == base, "no table is made or uploaded"
        ref = b.render(cam, W, H)
        for _ in range(2):
            ref = b.render(cam, W, H)
        after, after_b = a.render(cam, W, H), b.render(cam, W, H)
        assert after[0].tobytes() == before[0].tobytes() == after_b[0].tobytes() == ref[0].tobytes()
        assert a.last_render_path() == b.last_render_path() and path == 1, (path, a.last_render_path(), b.last_render_path())
        assert all(after[1][k] == before[1][k] == after_b[1][k] for k in KEYS)
        assert a.layout_hash() == b.layout_hash() and a.device_bytes() == b.device_bytes()
    finally:
        a.close()
        b.close()

"""GPU tests of signed distance and occupancy (include/cgrt.h cgrt_signed_distance*; Scene.sdf, sdf_device, sdf_tensor, sdf_grid and its
_device / _tensor forms, debug_sdf_work).

Everything is compared as bytes and no point is left out: the fused kernel (k_sdf), the Python compositions it replaces
(Scene.signed_distance_tensor / Scene.inside_tensor: three count_crossings launches, one closest_points launch and torch arithmetic) and
tests/sdf_ref.py -- the definition on the CPU, which tests/test_sdf_cpu.py holds to the analytic box distance -- give the same values.  The
point lists are closest_ref.mixed_queries (uniform, on the surface, at vertices, on edges, far; one NaN and one inf point): the on-plane
and through-edge points are where a parity goes wrong.  Device outputs lie between guards of sentinel bytes.

blob, monkey and dodge are OPEN meshes (tests/test_point_scale_cpu.py asserts it): on them "inside" has no geometric meaning, and these
tests pin the definition, not geometry.  The sign is held to geometry on the closed meshes (cube, dragon) in tests/test_point_scale_*.py."""
import dataclasses
import threading

import numpy as np
import pytest

import closest_ref as cr
import sdf_ref
from conftest import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
INF = float("inf")
LENGTHS = (1, 63, 64, 65, 129, 4097)
NMAX = max(LENGTHS)
FIVE_DIRS = ((0.31, -0.72, 0.62), (-0.81, 0.13, 0.57), (0.22, 0.64, -0.74), (-0.45, -0.55, -0.70), (0.93, 0.27, 0.25))


class Guarded:
    """nbytes of device memory between two guards, all of it sentinel bytes before the call."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.uint8, device="cuda")

    def tensor(self, dtype, shape):
        return self.buf[PAD : PAD + self.n].view(dtype).view(tuple(shape))

    def bytes(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()[PAD : PAD + self.n]

    def intact(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENTINEL).all() and (b[PAD + self.n :] == SENTINEL).all())


_scenes = {}
_refs = {}


@pytest.fixture(scope="module")
def scenes(pkg, scene_data):
    """name -> (SceneData, Scene on device 0), created once."""

    def get(name):
        if name not in _scenes:
            sd = scene_data(name)
            _scenes[name] = (sd, pkg.Scene(sd, device=0))
        return _scenes[name]

    yield get
    for _, sc in _scenes.values():
        sc.close()
    _scenes.clear()


def _queries(sd, name):
    if name not in _refs:
        _refs[name] = [cr.mixed_queries(sd, NMAX, 11), None]
    return _refs[name][0]


def _reference(pkg, orc, sd, name):
    """The definition on the CPU for the scene's whole query list, computed once."""
    q = _queries(sd, name)
    if _refs[name][1] is None:
        _refs[name][1] = sdf_ref.reference(orc, sd, q, pkg.INSIDE_DIRECTIONS)
    return _refs[name][1]


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _composition(sc, d_q, max_dist2=INF, directions=None):
    """What the fused entries replace, from the parent's own methods: (sdf, inside) as numpy."""
    inside = sc.inside_tensor(d_q, directions=directions)
    d2 = sc.closest_points_tensor(d_q, max_dist2=max_dist2)["dist2"]
    dist = torch.sqrt(d2)
    return _np(torch.where(inside, -dist, dist)), _np(inside)


def _assert_same(got, want, what, rows=None):
    (gs, gi), (ws, wi) = got, want
    if rows is not None:
        gs, gi, ws, wi = gs[rows], gi[rows], ws[rows], wi[rows]
    assert gs.dtype == np.float32 and gi.dtype == np.bool_ and gs.shape == ws.shape and gi.shape == wi.shape, what
    bad = np.flatnonzero(~same_bits(gs, ws) | (gi != wi))
    assert len(bad) == 0, (what, len(bad), int(bad[0]), gs[bad[0]], ws[bad[0]], gi[bad[0]], wi[bad[0]])


# ---- 1. the list form against the composition and the CPU reference ----
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["triangle", "cube", "cornell", "monkey", "blob"])
def test_list_form_against_the_composition_and_the_reference(pkg, orc, scenes, name, n):
    sd, sc = scenes(name)
    q = _queries(sd, name)[:n]
    ref = tuple(x[:n] for x in _reference(pkg, orc, sd, name))
    d_q = torch.from_numpy(q.copy()).cuda()
    s, i = sc.sdf_tensor(d_q)
    assert s.dtype == torch.float32 and i.dtype == torch.bool and s.shape == (n,) and i.shape == (n,)
    got = (_np(s), _np(i))
    finite = np.isfinite(q).all(axis=1)
    _assert_same(got, ref, (name, n, "fused against the CPU reference"))
    _assert_same(got, (_np(sc.signed_distance_tensor(d_q)), _np(sc.inside_tensor(d_q))), (name, n, "fused against the composition"), finite)
    _assert_same(sc.sdf(q), got, (name, n, "host form against the tensor form"))
    assert (np.signbit(got[0]) == got[1]).all(), "the sign is the vote (dist2 == 0 inside gives -0.0)"
    assert np.isposinf(got[0][~finite]).all() and not got[1][~finite].any()
    if n == NMAX and name != "triangle":
        on_surface = got[0][2::5][np.isfinite(q[2::5]).all(axis=1)]  # (family 2: exact vertex positions)
        assert (on_surface == 0).all()
        print(f"{name}: {int(got[1].sum())} of {n} inside, {int((np.signbit(on_surface)).sum())} of {len(on_surface)} at-vertex points voted inside")


# ---- 2. a scene too large for all pairs on the CPU ----
def test_dodge_against_the_composition(pkg, scenes):
    sd, sc = scenes("dodge")
    assert sc.num_subnodes() > 0, "the scene with in-leaf accelerators"
    q = cr.mixed_queries(sd, 4096, 11)
    finite = np.isfinite(q).all(axis=1)
    d_q = torch.from_numpy(q.copy()).cuda()
    s, i = sc.sdf_tensor(d_q)
    got = (_np(s), _np(i))
    _assert_same(got, (_np(sc.signed_distance_tensor(d_q)), _np(sc.inside_tensor(d_q))), "dodge", finite)
    _assert_same(sc.sdf(q), got, "dodge, host form")
    assert got[1].any() and (~got[1]).any()


# ---- 3. the radius ----
@pytest.mark.parametrize("name", ["cube", "blob"])
def test_max_dist2(pkg, scenes, name):
    sd, sc = scenes(name)
    q = _queries(sd, name)[:1024]
    finite = np.isfinite(q).all(axis=1)
    r2 = (0.25 * cr.scene_scale(sd)) ** 2
    d_q = torch.from_numpy(q.copy()).cuda()
    unbounded = tuple(_np(x) for x in sc.sdf_tensor(d_q))
    got = tuple(_np(x) for x in sc.sdf_tensor(d_q, max_dist2=r2))
    _assert_same(got, _composition(sc, d_q, max_dist2=r2), (name, "against the composition fed closest_points_tensor(max_dist2)"), finite)
    beyond = np.isinf(got[0]) & finite
    within = ~np.isinf(got[0])
    assert beyond.any() and within.any(), (name, int(beyond.sum()))
    assert (np.signbit(got[0]) == got[1]).all() and (got[1] == unbounded[1]).all(), "+-inf with the vote's sign; the vote does not depend on it"
    assert same_bits(got[0][within], unbounded[0][within]).all(), "within the radius the bytes are unchanged"
    assert (np.abs(unbounded[0][beyond]) ** 2 > np.float32(r2) * np.float32(0.999)).all()
    _assert_same(sc.sdf(q, max_dist2=r2), got, (name, "host form"))
    # max_dist2 == 0 still accepts dist2 == 0
    vq = cr.vertex_queries(sd, 64, 41)
    s0 = sc.sdf(vq, max_dist2=0.0, want="sdf")
    assert (s0 == 0).all()


# ---- 4. the directions ----
@pytest.mark.parametrize("dirs", [(FIVE_DIRS[0],), FIVE_DIRS], ids=["one", "five"])
def test_directions(pkg, scenes, dirs):
    for name in ("cube", "blob"):
        sd, sc = scenes(name)
        q = _queries(sd, name)[:1025]
        finite = np.isfinite(q).all(axis=1)
        d_q = torch.from_numpy(q.copy()).cuda()
        got = tuple(_np(x) for x in sc.sdf_tensor(d_q, directions=dirs))
        _assert_same(got, _composition(sc, d_q, directions=dirs), (name, len(dirs)), finite)
        assert (_np(sc.sdf_tensor(d_q, directions=dirs, want=("inside",))) == got[1]).all()
        assert (sc.sdf(q, directions=dirs, want="inside") == got[1]).all()


def test_default_directions_are_the_packages(pkg, scenes):
    sd, sc = scenes("blob")
    q = _queries(sd, "blob")[:1025]
    _assert_same(sc.sdf(q, directions=pkg.INSIDE_DIRECTIONS), sc.sdf(q), "ndirs = 0 against the three directions spelt out")


def test_bad_directions(pkg, scenes):
    sd, sc = scenes("cube")
    d_q = torch.zeros((8, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        sc.sdf_tensor(d_q, directions=FIVE_DIRS[:2])
    with pytest.raises(ValueError):
        sc.sdf_tensor(d_q, directions=FIVE_DIRS + FIVE_DIRS[:4])
    for bad in (((1, 0, 0), (0, 0, 0), (0, 1, 0)), ((1, float("nan"), 0),)):
        with pytest.raises((pkg.CgrtError, ValueError)) as e:
            sc.sdf_tensor(d_q, directions=bad)
        assert not isinstance(e.value, pkg.CgrtError) or e.value.code == -1
    prm = pkg.SdfParams()
    prm.max_dist2, prm.ndirs = INF, 2
    out = torch.zeros(8, dtype=torch.float32, device="cuda")
    import ctypes as C

    rc = pkg.lib().cgrt_signed_distance_device(sc._h, C.c_void_p(d_q.data_ptr()), 8, C.byref(prm), C.c_void_p(out.data_ptr()), None, None)
    assert rc == -1


# ---- 5. occupancy only ----
def test_occupancy_only(pkg, scenes):
    sd, sc = scenes("blob")
    n = 1025
    q = _queries(sd, "blob")[:n]
    d_q = torch.from_numpy(q.copy()).cuda()
    both = sc.sdf_tensor(d_q)
    g_s, g_i = Guarded(4 * n), Guarded(n)
    i = sc.sdf_tensor(d_q, want=("inside",), out=g_i.tensor(torch.bool, (n,)))
    assert i.dtype == torch.bool and (_np(i) == _np(both[1])).all()
    # the raw entry with no sdf pointer, the sdf buffer lying beside it untouched
    g_i2 = Guarded(n)
    sc.sdf_device(d_q.data_ptr(), n, 0, g_i2.tensor(torch.uint8, (n,)).data_ptr())
    assert (g_i2.bytes() == _np(both[1]).view(np.uint8)).all() and set(np.unique(g_i2.bytes())) <= {0, 1}
    assert (g_s.bytes() == SENTINEL).all() and g_s.intact() and g_i.intact() and g_i2.intact()
    assert (sc.sdf(q, want=("inside",)) == _np(both[1])).all()
    w = sc.debug_sdf_work(q, want_sdf=False)
    assert w[0] == 0 and w[1] == 0 and w[2] > 0 and w[3] > 0, w
    w = sc.debug_sdf_work(q, want_sdf=True)
    assert w[0] > 0 and w[1] > 0, w
    assert (w[0], w[1]) == sc.debug_closest_work(q), "phase 1 is the closest-point search, step for step"


# ---- 6. the early end of the vote ----
def test_early_end_of_the_vote(pkg, scenes):
    sd, sc = scenes("cube")
    far = cr.far_queries(sd, 1000, 5)
    d_far = torch.from_numpy(far.copy()).cuda()
    counts = [int(_np(sc.count_crossings_tensor(torch.cat([d_far, torch.tensor(d, dtype=torch.float32, device="cuda").expand(len(far), 3),
                                                                  torch.full((len(far), 1), INF, device="cuda")], dim=1).contiguous())).sum())
              for d in pkg.INSIDE_DIRECTIONS[:2]]
    assert counts == [0, 0], "far outside the cube the first two rays cross nothing"
    w = sc.debug_sdf_work(far)
    assert w[4] == 2 * len(far), w
    got = tuple(_np(x) for x in sc.sdf_tensor(d_far))
    _assert_same(got, (_np(sc.signed_distance_tensor(d_far)), _np(sc.inside_tensor(d_far))), "far points")
    assert not got[1].any()
    for name in ("cube", "blob"):
        sd, sc = scenes(name)
        q = _queries(sd, name)
        nf = int(np.isfinite(q).all(axis=1).sum())
        w = sc.debug_sdf_work(q)
        print(f"{name}: {w[4] / nf:.3f} direction walks per finite point")
        assert 2 * nf <= w[4] <= 3 * nf, (name, w)
        assert sc.debug_sdf_work(q, directions=(FIVE_DIRS[0],))[4] == nf


# ---- 7. the other search paths ----
def test_linear_leaves(pkg, scenes):
    sd, accel = scenes("dodge")
    q = cr.mixed_queries(sd, 1024, 11)
    finite = np.isfinite(q).all(axis=1)
    try:
        pkg.set_leaf_accel(False)
        sc = pkg.Scene(sd, device=0)
    finally:
        pkg.set_leaf_accel(True)
    try:
        assert sc.num_subnodes() == 0
        d_q = torch.from_numpy(q.copy()).cuda()
        got = tuple(_np(x) for x in sc.sdf_tensor(d_q))
        _assert_same(got, (_np(sc.signed_distance_tensor(d_q)), _np(sc.inside_tensor(d_q))), "linear leaves", finite)
        _assert_same(got, accel.sdf(q), "linear leaves against the accelerated scene")
    finally:
        sc.close()


def test_nan_and_inf_vertices_take_the_brute_parity_path(pkg, scenes):
    clean, _ = scenes("blob")
    pos = np.asarray(clean.pos_nrm, np.float32).reshape(-1, 6).copy()
    tri = np.asarray(clean.tri).reshape(-1, 3)
    pos[tri[100, 1], 0] = np.nan
    pos[tri[900, 2], 1] = np.inf
    sd = dataclasses.replace(clean, pos_nrm=pos, name="blob+nan+inf")
    q = _queries(clean, "blob")[:1024]
    finite = np.isfinite(q).all(axis=1)
    sc = pkg.Scene(sd, device=0)
    try:
        d_q = torch.from_numpy(q.copy()).cuda()
        got = tuple(_np(x) for x in sc.sdf_tensor(d_q))
        _assert_same(got, (_np(sc.signed_distance_tensor(d_q)), _np(sc.inside_tensor(d_q))), "blob+nan+inf", finite)
        w = sc.debug_sdf_work(q, want_sdf=False)
        assert w[2] == 0 and w[3] == w[4] * sd.ntris, ("every walk tests every triangle", w)
    finally:
        sc.close()


# ---- 8. special points and scenes ----
def test_special_points(pkg, scenes):
    sd, sc = scenes("cube")
    lo, hi = cr.scene_box(sd)
    q = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.inf, -np.inf], 0.5 * (lo + hi)], np.float32)
    s, i = sc.sdf(q)
    assert np.isposinf(s[:4]).all() and not i[:4].any() and not np.signbit(s[:4]).any()
    assert i[4] and s[4] < 0, "the cube's centre"
    s, i = (_np(x) for x in sc.sdf_tensor(torch.from_numpy(q).cuda()))
    assert np.isposinf(s[:4]).all() and not i[:4].any() and i[4]


def test_a_scene_without_meshes(pkg, scene_data):
    sd = scene_data("spheres")
    assert sd.ntris == 0 and len(sd.spheres) > 0
    sc = pkg.Scene(sd, device=0)
    try:
        q = np.random.default_rng(3).normal(size=(130, 3)).astype(np.float32)
        for s, i in (sc.sdf(q), sc.sdf(q, max_dist2=4.0), sc.sdf_grid((-1, -1, -1), (0.5, 0.5, 0.5), (5, 4, 3))):
            assert np.isposinf(s).all() and not i.any()
        assert sc.debug_sdf_work(q) == (0, 0, 0, 0, 0)
    finally:
        sc.close()


# ---- 9. the device form ----
@pytest.mark.parametrize("n", (1, 65, 4097))
def test_device_form_between_guards_on_a_side_stream(pkg, orc, scenes, n):
    sd, sc = scenes("blob")
    q = _queries(sd, "blob")[:n]
    ref = tuple(x[:n] for x in _reference(pkg, orc, sd, "blob"))
    d_q = torch.from_numpy(q.copy()).cuda()
    g_s, g_i = Guarded(4 * n), Guarded(n)
    out_s, out_i = g_s.tensor(torch.float32, (n,)), g_i.tensor(torch.bool, (n,))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    s, i = sc.sdf_tensor(d_q, out=(out_s, out_i), stream=side)
    side.synchronize()
    assert s is out_s and i is out_i, "out= is returned as passed"
    assert g_s.intact() and g_i.intact()
    _assert_same((_np(s), _np(i)), ref, ("device form", n))
    assert set(np.unique(g_i.bytes())) <= {0, 1}
    with pytest.raises(ValueError):
        sc.sdf_tensor(d_q, out=(torch.zeros(n + 1, dtype=torch.float32, device="cuda"), out_i))
    with pytest.raises(ValueError):
        sc.sdf_tensor(d_q.cpu())


def test_device_form_checks_its_buffers(pkg, scenes):
    import ctypes as C

    sd, sc = scenes("cube")
    d_q = torch.zeros((16, 3), dtype=torch.float32, device="cuda")
    d_s = torch.zeros(16, dtype=torch.float32, device="cuda")
    d_i = torch.zeros(16, dtype=torch.uint8, device="cuda")
    host = np.zeros(64, np.float32)
    sc.sdf_device(d_q.data_ptr(), 16, d_s.data_ptr(), d_i.data_ptr())
    torch.cuda.synchronize()
    before = (_np(d_s).copy(), _np(d_i).copy())
    for args in ((host.ctypes.data, 16, d_s.data_ptr(), d_i.data_ptr()), (d_q.data_ptr(), 16, host.ctypes.data, d_i.data_ptr()),
                 (d_q.data_ptr(), 16, d_s.data_ptr(), host.ctypes.data)):
        with pytest.raises(pkg.CgrtError) as e:
            sc.sdf_device(*args)
        assert e.value.code == -1, args
    with pytest.raises(pkg.CgrtError) as e:
        sc.sdf_grid_device((0, 0, 0), (1, 1, 1), (4, 2, 2), host.ctypes.data, d_i.data_ptr())
    assert e.value.code == -1
    # too short: allocations of their own (a torch tensor lies in a larger block of torch's allocator), 4 KiB where n asks for megabytes
    n = 1 << 22
    hip = C.CDLL(pkg.LIB_PATH)
    big_q = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    big_s = torch.zeros(n, dtype=torch.float32, device="cuda")
    big_i = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), C.c_size_t(4096)) == 0
    try:
        for args in ((small.value, n, big_s.data_ptr(), big_i.data_ptr()), (big_q.data_ptr(), n, small.value, big_i.data_ptr()),
                     (big_q.data_ptr(), n, big_s.data_ptr(), small.value), (big_q.data_ptr(), n, 0, small.value)):
            with pytest.raises(pkg.CgrtError) as e:
                sc.sdf_device(*args)
            assert e.value.code == -1, args
        for ds, di in ((small.value, big_i.data_ptr()), (big_s.data_ptr(), small.value)):
            with pytest.raises(pkg.CgrtError) as e:
                sc.sdf_grid_device((0, 0, 0), (1, 1, 1), (n >> 8, 16, 16), ds, di)
            assert e.value.code == -1
        assert not big_s.any() and not big_i.any(), "refused before any work"
    finally:
        assert hip.hipFree(small) == 0
    assert (before[0] == _np(d_s)).all() and (before[1] == _np(d_i)).all(), "refused before any work"
    sc.sdf_device(0, 0, d_s.data_ptr(), 0)  # n == 0 touches nothing


# ---- 10. grids ----
GRID_DIMS = ((1, 1, 1), (5, 3, 2), (9, 4, 5), (64, 1, 1), (3, 70, 2))


def _grids(sd, name):
    lo, hi = cr.scene_box(sd)
    ext = hi - lo
    for dims in GRID_DIMS:
        spacing = 1.3 * ext / np.maximum(np.asarray(dims) - 1, 1)
        yield name, tuple(lo - 0.15 * ext), tuple(spacing), dims
    yield name + ", negative and zero spacing", tuple(hi + 0.1 * ext), (-0.11 * ext[0], 0.0, 0.3 * ext[2]), (9, 4, 5)


@pytest.mark.parametrize("name", ["cube", "blob"])
def test_grids(pkg, scenes, name):
    sd, sc = scenes(name)
    cases = list(_grids(sd, name))
    if name == "cube":  # points exactly on faces, edges and corners (the cube spans -0.5 .. 0.5 or a multiple of the spacing)
        lo, hi = cr.scene_box(sd)
        assert (np.abs(lo / 0.25) % 1 == 0).all() and (np.abs(hi / 0.25) % 1 == 0).all()
        m = int(max(np.abs(lo).max(), np.abs(hi).max()) / 0.25) + 2
        cases.append(("cube, origin 0 and spacing 0.25", (0.0, 0.0, 0.0), (0.25, 0.25, 0.25), (m, m, m)))
        cases.append(("cube, lattice through it", tuple(lo - 0.25), (0.25, 0.25, 0.25), tuple(int(x) for x in ((hi - lo) / 0.25 + 3))))
    for what, origin, spacing, dims in cases:
        nx, ny, nz = dims
        pts = pkg.sdf_grid_points(origin, spacing, dims)
        want = sc.sdf(pts)
        g_s, g_i = Guarded(4 * len(pts)), Guarded(len(pts))
        s, i = sc.sdf_grid_tensor(origin, spacing, dims, out=(g_s.tensor(torch.float32, (nz, ny, nx)), g_i.tensor(torch.bool, (nz, ny, nx))))
        assert s.shape == (nz, ny, nx) and i.shape == (nz, ny, nx)
        got = (_np(s), _np(i))
        assert g_s.intact() and g_i.intact(), what
        _assert_same((got[0].reshape(-1), got[1].reshape(-1)), want, (what, dims, "grid against the list form on sdf_grid_points"))
        host = sc.sdf_grid(origin, spacing, dims)
        assert host[0].shape == (nz, ny, nx) and host[1].shape == (nz, ny, nx)
        _assert_same(host, got, (what, dims, "host grid form against the device grid form"))
        try:  # the other lane mapping: the same bytes
            pkg._check(pkg.lib().cgrt_debug_set_sdf_grid_mapping(1))
            _assert_same(sc.sdf_grid(origin, spacing, dims), got, (what, dims, "linear lane mapping"))
        finally:
            pkg._check(pkg.lib().cgrt_debug_set_sdf_grid_mapping(0))
        only = sc.sdf_grid_tensor(origin, spacing, dims, want="inside")
        assert (_np(only) == got[1]).all()
        if "spacing 0.25" in what or "lattice" in what:
            assert (got[0] == 0).sum() >= 8, "grid points on the surface"
            assert got[1].any() and (~got[1]).any()


# ---- 11. threads ----
def test_four_threads_on_one_scene(pkg, scenes):
    sd, sc = scenes("blob")
    q = _queries(sd, "blob")
    single = tuple(x.tobytes() for x in sc.sdf(q))
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                results[k] = tuple(x.tobytes() for x in sc.sdf(q))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(r == single for r in results), "the host form is concurrent on one scene"

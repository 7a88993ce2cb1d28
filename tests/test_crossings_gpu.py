"""GPU tests of the crossing queries (include/cgrt.h cgrt_count_crossings*, cgrt_list_crossings*; Scene.count_crossings, list_crossings,
first_crossings and their _brute / _device / _tensor forms, debug_crossing_work, inside_tensor, signed_distance_tensor).

Everything is compared as bytes: the device's tree search (k_crossings), the device's brute force and tests/crossings_ref.py -- the CPU
oracle's intersectRayWithTriangle over all ray x triangle pairs, sorted and slotted, which tests/test_crossings_cpu.py holds to the
oracle's brute-force intersect and to a float64 referee -- give the same counts and the same records.  The ray lists interleave the
families of crossings_ref (camera frame, random, origins at vertices, through edges and vertices, segments ending exactly on a crossing,
t = 0, a zero direction component) and carry one NaN and one inf ray.  Device outputs lie between guards of sentinel bytes."""
import dataclasses
import threading

import numpy as np
import pytest

import crossings_ref as xr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5
PAD = 256
LENGTHS = (1, 63, 64, 65, 4097)
NMAX = max(LENGTHS)
KS = (1, 2, 4)


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


def _records(t):
    torch.cuda.synchronize()
    return np.ascontiguousarray(t.cpu().numpy()).view(xr.CROSSING_DTYPE).reshape(t.shape[:-1])


def _first_difference(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    if a.shape != b.shape:
        return "shapes", a.shape, b.shape
    d = np.flatnonzero((a["t"].view(np.uint32) != b["t"].view(np.uint32)) | (a["prim_id"] != b["prim_id"]))
    return None if len(d) == 0 else (int(d[0]), a[d[0]], b[d[0]])


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


def _mixed(pkg, orc, sd, name):
    """The scene's one ray list (NMAX mixed rays) and its ground truth, computed once."""
    if name not in _refs:
        rays = xr.mixed_rays(pkg, orc, sd, NMAX, 11)
        _refs[name] = (rays, xr.reference(orc, sd, rays))
    return _refs[name]


def _prefix(ref, n):
    counts, offsets, rec = ref
    return counts[:n], offsets[: n + 1], rec[: offsets[n]]


def _big_rays(pkg, orc, sd, seed):
    """4 096 rays for the scenes that are too large for all pairs: camera frame, random, through edges and vertices, origins at vertices."""
    return np.concatenate([xr.camera_rays(pkg, orc, 1024), xr.random_rays(sd, 2048, seed), xr.edge_and_vertex_rays(sd, 512, seed + 1),
                           xr.vertex_origin_rays(sd, 512, seed + 2)])


def _assert_tree_equals_brute(sc, rays, ks=(4,)):
    counts = sc.count_crossings(rays)
    off_t, rec_t = sc.list_crossings(rays)
    off_b, rec_b = sc.list_crossings_brute(rays)
    assert (off_t == off_b).all(), "counts of the tree search against brute force"
    assert (np.diff(off_t) == counts).all()
    assert xr.same_records(rec_t, rec_b), _first_difference(rec_t, rec_b)
    for k in ks:
        ft, ct = sc.first_crossings(rays, k)
        fb, cb = sc.list_crossings_brute(rays, k=k)
        assert (ct == counts).all() and (cb == counts).all(), k
        assert xr.same_records(ft, fb), (k, _first_difference(ft, fb))
        # without counts a full slot's bound shrinks to the largest t kept: the same records
        fs, none = sc.first_crossings(rays, k, want_counts=False)
        assert none is None and xr.same_records(fs, fb), (k, "shrinking bound", _first_difference(fs, fb))
    # slots of mixed sizes, without counts: full slots shrink their bound, the others do not
    sizes = np.random.default_rng(9).choice([0, 1, 2, 3, 8], len(rays))
    slots = np.zeros(len(rays) + 1, np.int64)
    np.cumsum(sizes, out=slots[1:])
    want, _ = sc.list_crossings_brute(rays, offsets=slots)
    got, none = sc.list_crossings(rays, offsets=slots, want_counts=False)
    assert none is None and xr.same_records(got, want), ("slots, shrinking bound", _first_difference(got, want))
    assert ((sizes > 0) & (sizes < counts)).any(), "some slots are shorter than their ray's count"
    return counts, off_t, rec_t


# ---- 1. parity: tree == brute == ground truth ----
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("name", ["triangle", "cube", "cornell", "monkey", "blob"])
def test_tree_brute_and_ground_truth_agree(pkg, orc, scenes, name, n):
    sd, sc = scenes(name)
    rays, ref = _mixed(pkg, orc, sd, name)
    rays, ref = rays[:n], _prefix(ref, n)
    counts, offsets, rec = ref
    assert (sc.count_crossings(rays) == counts).all(), (name, n, "counts")
    off_b, rec_b = sc.list_crossings_brute(rays)
    assert (off_b == offsets).all() and xr.same_records(rec_b, rec), (name, n, "brute force against the ground truth", _first_difference(rec_b, rec))
    off_t, rec_t = sc.list_crossings(rays)
    assert off_t.dtype == np.int64 and rec_t.dtype == pkg.CROSSING_DTYPE
    assert (off_t == offsets).all() and xr.same_records(rec_t, rec), (name, n, "tree search against the ground truth", _first_difference(rec_t, rec))
    for k in KS:
        want = xr.first_k(ref, k)
        ft, ct = sc.first_crossings(rays, k)
        fb, cb = sc.list_crossings_brute(rays, k=k)
        assert (ct == counts).all() and (cb == counts).all(), (name, n, k, "the full counts beside short slots")
        assert xr.same_records(fb, want), (name, n, k, "brute force", _first_difference(fb, want))
        assert xr.same_records(ft, want), (name, n, k, "tree search", _first_difference(ft, want))
    if n == NMAX and name != "triangle":
        assert counts.max() >= 2 and (counts == 0).any()
        t, ray = rec["t"], np.repeat(np.arange(n), counts)
        same = ray[1:] == ray[:-1]
        assert (t[1:][same] >= t[:-1][same]).all(), "ordered by t"


def test_dodge_tree_equals_brute(pkg, orc, scenes):
    sd, sc = scenes("dodge")
    assert sc.num_subnodes() > 0, "the scene with in-leaf accelerators"
    _assert_tree_equals_brute(sc, _big_rays(pkg, orc, sd, 21), ks=(1, 4))


@pytest.fixture(scope="module")
def dragon(pkg):
    sd = pkg.scenes.make_dragon(200_000)
    sc = pkg.Scene(sd, device=0)
    yield sd, sc
    sc.close()


def test_dragon_tree_equals_brute_and_the_ground_truth_on_64_rays(pkg, orc, dragon):
    """Leaves of more than 32 triangles: the accelerators are exercised (no committed scene does that)."""
    sd, sc = dragon
    assert sc.num_subnodes() > 0
    rays = _big_rays(pkg, orc, sd, 31)
    counts, offsets, rec = _assert_tree_equals_brute(sc, rays, ks=(2,))
    pick = np.arange(0, len(rays), len(rays) // 64)[:64]
    c64, o64, r64 = xr.reference(orc, sd, rays[pick])
    assert (counts[pick] == c64).all()
    got = np.concatenate([rec[offsets[i] : offsets[i + 1]] for i in pick])
    assert xr.same_records(got, r64), _first_difference(got, r64)
    assert counts.max() >= 4


def test_work_counters(pkg, orc, dragon):
    sd, sc = dragon
    rays = _big_rays(pkg, orc, sd, 31)
    nodes, tris = sc.debug_crossing_work(rays)
    print(f"dragon, {len(rays)} rays: {nodes / len(rays):.1f} node steps and {tris / len(rays):.1f} triangles evaluated per ray of {sd.ntris}")
    assert nodes > 0 and 0 < tris < len(rays) * sd.ntris, "the boxes cull"


# ---- 2. configurations: the same bytes ----
def test_linear_leaves_no_fast_tree_exact_walk_and_kernel_shapes(pkg, orc, scenes):
    sd, default = scenes("dodge")
    rays = _big_rays(pkg, orc, sd, 21)[::4]
    want_off, want = default.list_crossings_brute(rays)
    want4, _ = default.list_crossings_brute(rays, k=4)

    def check(sc, what):
        off, rec = sc.list_crossings(rays)
        assert (off == want_off).all() and xr.same_records(rec, want), (what, _first_difference(rec, want))
        f4, c4 = sc.first_crossings(rays, 4)
        assert xr.same_records(f4, want4) and (c4 == np.diff(want_off)).all(), what

    try:
        pkg.set_leaf_accel(False)
        sc = pkg.Scene(sd, device=0)
    finally:
        pkg.set_leaf_accel(True)
    try:
        assert sc.num_subnodes() == 0
        check(sc, "linear leaves")
    finally:
        sc.close()
    try:
        pkg.set_fast_tree(0)
        sc = pkg.Scene(sd, device=0)
    finally:
        pkg.set_fast_tree(-1)
    try:
        check(sc, "no fast tree")
    finally:
        sc.close()
    walk = default.walk()
    try:
        default.set_walk(False)
        check(default, "exact walk")
    finally:
        default.set_walk(bool(walk))
    try:
        for mode in (-1, 0, 1, 2, 3):
            pkg.set_kernel_shape(mode)
            check(default, f"kernel shape {mode}")
    finally:
        pkg.set_kernel_shape(-1)


def test_wild_leaves_fall_back_to_brute_force(pkg, orc, scenes):
    """The blob scaled by 2^38: triangle planes leave float32's range, the builder marks wild leaves and the whole call tests every triangle."""
    small, _ = scenes("blob")
    pn = np.asarray(small.pos_nrm, np.float32).reshape(-1, 6).copy()
    pn[:, 0:3] *= np.float32(2.0 ** 38)
    sd = dataclasses.replace(small, pos_nrm=pn, name="blob*2^38")
    sc = pkg.Scene(sd, device=0)
    try:
        assert sc.build_info()["wild_leaves"] > 0
        rays = np.concatenate([xr.random_rays(sd, 384, 5), xr.edge_and_vertex_rays(sd, 64, 6), xr.vertex_origin_rays(sd, 64, 7)])
        ref = xr.reference(orc, sd, rays)
        off, rec = sc.list_crossings(rays)
        assert (off == ref[1]).all() and xr.same_records(rec, ref[2]), _first_difference(rec, ref[2])
        off_b, rec_b = sc.list_crossings_brute(rays)
        assert (off_b == ref[1]).all() and xr.same_records(rec_b, ref[2])
        f2, c2 = sc.first_crossings(rays, 2)
        assert xr.same_records(f2, xr.first_k(ref, 2)) and (c2 == ref[0]).all()
        assert sc.debug_crossing_work(rays) == (0, len(rays) * sd.ntris), "every triangle for every ray, no node steps"
    finally:
        sc.close()


def test_spheres_are_ignored_and_a_scene_without_meshes_has_no_crossings(pkg, orc, scenes, scene_data):
    sd, plain = scenes("blob")
    rays, ref = _mixed(pkg, orc, sd, "blob")
    rays, ref = rays[:512], _prefix(ref, 512)
    hi = xr.positions(sd).max(0)
    sph = np.asarray([[hi[0], hi[1], 0.0, 0.45 * hi[0], -1], [-hi[0], 0.0, hi[2], 0.4 * hi[0], 0]], np.float32)
    sc = pkg.Scene(dataclasses.replace(sd, spheres=sph, name="blob+spheres"), device=0)
    try:
        off, rec = sc.list_crossings(rays)
        assert (off == ref[1]).all() and xr.same_records(rec, ref[2])
    finally:
        sc.close()
    empty = pkg.Scene(scene_data("spheres"), device=0)
    try:
        assert not empty.count_crossings(rays).any()
        f, c = empty.first_crossings(rays, 2)
        assert xr.same_records(f, xr.unused(2 * len(rays)).reshape(-1, 2)) and not c.any()
        assert empty.debug_crossing_work(rays) == (0, 0)
    finally:
        empty.close()


def test_empty_lists_as_the_first_host_call_on_a_fresh_scene(pkg, scene_data):
    """No ray crosses anything and no count is asked for: there is nothing to write, and the call lane has no buffers yet."""
    sd = scene_data("cube")
    lo, hi = xr.grown_box(sd)
    n = 100
    away = np.zeros((n, 7), np.float32)
    away[:, 0:3], away[:, 3:6], away[:, 6] = hi + 1.0, (1.0, 2.0, 3.0), xr.FMAX  # beyond the box, pointing away from it
    zeros = np.zeros(n + 1, np.int64)

    def fresh(call):
        sc = pkg.Scene(sd, device=0)
        try:
            return call(sc)
        finally:
            sc.close()

    off, rec = fresh(lambda sc: sc.list_crossings(away))
    assert off.shape == (n + 1,) and not off.any() and rec.shape == (0,) and rec.dtype == pkg.CROSSING_DTYPE
    rec, none = fresh(lambda sc: sc.list_crossings(away, offsets=zeros, want_counts=False))
    assert rec.shape == (0,) and none is None
    rec, counts = fresh(lambda sc: sc.list_crossings(away, offsets=zeros))
    assert rec.shape == (0,) and counts.shape == (n,) and not counts.any()
    rec, counts = fresh(lambda sc: sc.list_crossings_brute(away, offsets=zeros))
    assert rec.shape == (0,) and not counts.any()
    # empty slots of rays that DO cross: still nothing to write, the counts are the full ones
    through = away.copy()
    through[:, 0:3], through[:, 3:6] = lo - 1.0, (hi - lo) + 2.0  # along the box's diagonal
    rec, counts = fresh(lambda sc: sc.list_crossings(through, offsets=zeros))
    assert rec.shape == (0,) and (counts >= 2).all()
    assert fresh(lambda sc: sc.list_crossings(through, offsets=zeros, want_counts=False))[0].shape == (0,)


# ---- 3. slots ----
def test_slots_shorter_than_the_count_keep_the_smallest(pkg, orc, scenes):
    sd, sc = scenes("monkey")
    rays, ref = _mixed(pkg, orc, sd, "monkey")
    rays, ref = rays[:1024], _prefix(ref, 1024)
    rng = np.random.default_rng(3)
    sizes = rng.choice([0, 0, 1, 2, 3, 8], len(rays))
    slots = np.zeros(len(rays) + 1, np.int64)
    np.cumsum(sizes, out=slots[1:])
    want = xr.slotted(ref, slots)
    got, counts = sc.list_crossings(rays, offsets=slots)
    assert (counts == ref[0]).all(), "counts are the full numbers whatever the slots hold"
    assert xr.same_records(got, want), _first_difference(got, want)
    assert ((sizes < ref[0]) & (sizes > 0)).any() and ((sizes > ref[0]) & (ref[0] > 0)).any() and (sizes == 0).any()
    out, _ = sc.list_crossings_brute(rays, offsets=slots)
    assert xr.same_records(out, want)
    # without counts the search may stop early (the bound shrinks to the largest t kept): the same records
    out, none = sc.list_crossings(rays, offsets=slots, want_counts=False)
    assert none is None and xr.same_records(out, want), _first_difference(out, want)
    for k in KS:
        out, none = sc.first_crossings(rays, k, want_counts=False)
        assert none is None and xr.same_records(out, xr.first_k(ref, k)), k


def test_no_offset_table_makes_the_device_form_write_outside_capacity(pkg, orc, scenes):
    sd, sc = scenes("cornell")
    rays, ref = _mixed(pkg, orc, sd, "cornell")
    counts, offsets, rec = ref
    pick = np.flatnonzero(counts >= 2)[:8]
    assert len(pick) == 8
    rays = np.ascontiguousarray(rays[pick])
    capacity = 12
    # pairs: 0 (7, 7) empty; 1 (7, 1) decreasing; 2 [1, 5); 3 (5, 5) empty; 4 [5, 9); 5 [9, 13) -> [9, 12); 6 [13, 20) beyond; 7 (20, 7) beyond
    # and decreasing.  Record 0 belongs to no slot.
    table = np.array([7, 7, 1, 5, 5, 9, 13, 20, 7], np.int64)
    assert len(table) == len(rays) + 1
    want = np.full(capacity * 8, SENTINEL, np.uint8).view(xr.CROSSING_DTYPE)
    for i, (b, e) in enumerate(zip(table[:-1], table[1:])):
        e = max(b, e)
        b, e = min(b, capacity), min(e, capacity)
        m = min(e - b, int(counts[pick[i]]))
        want[b : b + m] = rec[offsets[pick[i]] : offsets[pick[i]] + m]
        want[b + m : e] = xr.unused(e - b - m)
    d_rays = torch.from_numpy(rays).cuda()
    d_off = torch.from_numpy(table).cuda()
    g = Guarded(capacity * 8)
    gc = Guarded(len(rays) * 4)
    out = g.tensor(torch.float32, (capacity, 2))
    sc.list_crossings_device(d_rays.data_ptr(), len(rays), out.data_ptr(), capacity, d_offsets_ptr=d_off.data_ptr(),
                             d_counts_ptr=gc.tensor(torch.int32, (len(rays),)).data_ptr())
    assert g.intact() and gc.intact()
    assert g.bytes().tobytes() == want.tobytes(), _first_difference(g.bytes().view(xr.CROSSING_DTYPE), want)
    assert (gc.bytes().view(np.uint32) == counts[pick]).all()
    # a capacity of zero: nothing is written at all
    g0 = Guarded(capacity * 8)
    sc.list_crossings_device(d_rays.data_ptr(), len(rays), g0.tensor(torch.float32, (capacity, 2)).data_ptr(), 0, d_offsets_ptr=d_off.data_ptr())
    assert g0.intact() and (g0.bytes() == SENTINEL).all()


# ---- 4. host, device and tensor forms ----
@pytest.mark.parametrize("n", LENGTHS)
def test_device_and_tensor_forms_between_guards(pkg, orc, scenes, n):
    sd, sc = scenes("blob")
    rays, ref = _mixed(pkg, orc, sd, "blob")
    rays, ref = np.ascontiguousarray(rays[:n]), _prefix(ref, n)
    counts, offsets, rec = ref
    d_rays = torch.from_numpy(rays).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    gc = Guarded(4 * n)
    c = sc.count_crossings_tensor(d_rays, out=gc.tensor(torch.int32, (n,)), stream=side)
    side.synchronize()
    assert gc.intact() and (c.cpu().numpy().view(np.uint32) == counts).all()
    off, records = sc.list_crossings_tensor(d_rays, stream=side)
    side.synchronize()
    assert off.dtype == torch.int64 and (off.cpu().numpy() == offsets).all()
    assert records.shape == (len(rec), 2) and xr.same_records(_records(records), rec)
    for k in KS:
        g = Guarded(8 * n * k)
        out = g.tensor(torch.float32, (n, k, 2))
        f, fc = sc.first_crossings_tensor(d_rays, k, out=out, stream=side)
        side.synchronize()
        assert f is out and g.intact()
        assert xr.same_records(_records(out), xr.first_k(ref, k)) and (fc.cpu().numpy().view(np.uint32) == counts).all()
    # the raw device form on the current stream, full CSR list between guards
    g = Guarded(8 * len(rec))
    sc.list_crossings_device(d_rays.data_ptr(), n, g.tensor(torch.float32, (len(rec), 2)).data_ptr() if len(rec) else d_rays.data_ptr(), len(rec),
                             d_offsets_ptr=off.data_ptr())
    assert g.intact() and g.bytes().tobytes() == rec.tobytes()
    with pytest.raises(ValueError):
        sc.count_crossings_tensor(d_rays.cpu())
    with pytest.raises(ValueError):
        sc.first_crossings_tensor(d_rays, 2, out=torch.zeros((n, 3, 2), dtype=torch.float32, device="cuda"))


def test_device_forms_check_their_buffers(pkg, scenes):
    sd, sc = scenes("cube")
    d_r = torch.zeros((16, 7), dtype=torch.float32, device="cuda")
    d_o = torch.zeros((16, 2, 2), dtype=torch.float32, device="cuda")
    d_c = torch.zeros((16,), dtype=torch.int32, device="cuda")
    host = np.zeros((64,), np.float32)
    sc.count_crossings_device(d_r.data_ptr(), 16, d_c.data_ptr())
    sc.first_crossings_device(d_r.data_ptr(), 16, 2, d_o.data_ptr(), d_counts_ptr=d_c.data_ptr())
    torch.cuda.synchronize()
    refused = {
        "counts on the host": lambda: sc.count_crossings_device(d_r.data_ptr(), 16, host.ctypes.data),
        "records on the host": lambda: sc.first_crossings_device(d_r.data_ptr(), 16, 2, host.ctypes.data),
        "a list's counts on the host": lambda: sc.first_crossings_device(d_r.data_ptr(), 16, 2, d_o.data_ptr(), d_counts_ptr=host.ctypes.data),
        "offsets on the host": lambda: sc.list_crossings_device(d_r.data_ptr(), 16, d_o.data_ptr(), 32, d_offsets_ptr=host.ctypes.data),
        "rays on the host": lambda: sc.count_crossings_device(host.ctypes.data, 8, d_c.data_ptr()),
    }
    for what, call in refused.items():
        code = None
        try:
            call()
        except pkg.CgrtError as e:
            code = e.code
        assert code == -1, what
    sc.count_crossings_device(0, 0, 0)  # n == 0 touches nothing


def test_two_streams_and_four_threads_on_one_scene(pkg, orc, scenes):
    sd, sc = scenes("blob")
    rays, ref = _mixed(pkg, orc, sd, "blob")
    counts, offsets, rec = ref
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    a = [sc.first_crossings_tensor(d_rays, 4, stream=s1) for _ in range(2)]
    b = [sc.count_crossings_tensor(d_rays, stream=s2) for _ in range(2)]
    s1.synchronize()
    s2.synchronize()
    for f, c in a:
        assert xr.same_records(_records(f), xr.first_k(ref, 4)) and (c.cpu().numpy().view(np.uint32) == counts).all()
    for c in b:
        assert (c.cpu().numpy().view(np.uint32) == counts).all()
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                off, r = sc.list_crossings(rays)
                results[k] = off.tobytes() + r.tobytes()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(r == offsets.tobytes() + rec.tobytes() for r in results), "the host form is concurrent on one scene"


# ---- 5. the consequences ----
@pytest.mark.parametrize("name", ["cube", "cornell", "monkey", "blob"])
def test_first_crossing_is_the_brute_force_hit(pkg, orc, scenes, name):
    sd, sc = scenes(name)
    assert len(np.asarray(sd.spheres).reshape(-1)) == 0
    rays, ref = _mixed(pkg, orc, sd, name)
    first, counts = sc.first_crossings(rays, 1)
    hits, _ = sc.intersect_brute(rays, mesh=-1, want_normals=False)
    off, rec = sc.list_crossings(rays)
    on_plane = np.zeros(len(rays), bool)
    on_plane[np.repeat(np.arange(len(rays)), counts)[rec["t"] == 0]] = True
    use = ~on_plane
    assert ((counts[use] > 0) == (hits["hit"][use] != 0)).all()
    h = use & (counts > 0)
    assert (first["t"][h, 0].view(np.uint32) == hits["t"][h].view(np.uint32)).all() and (first["prim_id"][h, 0] == hits["prim_id"][h]).all()


def test_inside_and_signed_distance_on_the_cube(pkg, scenes):
    sd, sc = scenes("cube")
    p = xr.positions(sd)
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    rng = np.random.default_rng(78)
    ext = hi - lo
    pts = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (4096, 3)).astype(np.float32)
    q = pts.astype(np.float64)
    out = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    inside = (out == 0).all(axis=1)
    sdf = np.where(inside, -np.minimum(q - lo, hi - q).min(axis=1), np.sqrt((out * out).sum(axis=1)))
    keep = np.abs(sdf) > 1e-3
    d_pts = torch.from_numpy(pts).cuda()
    got_in = sc.inside_tensor(d_pts).cpu().numpy()
    got_sd = sc.signed_distance_tensor(d_pts).cpu().numpy()
    assert got_in.dtype == np.bool_ and got_sd.dtype == np.float32
    assert (got_in[keep] == inside[keep]).all() and inside[keep].any() and (~inside[keep]).any()
    assert np.abs(got_sd[keep] - sdf[keep]).max() <= 1e-5, float(np.abs(got_sd[keep] - sdf[keep]).max())
    with pytest.raises(ValueError):
        sc.inside_tensor(d_pts, directions=[[1, 2, 3], [3, 2, 1]])
